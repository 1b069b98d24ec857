// Undirected device graphs: row sort, transpose and symmetrisation of a device CSR.  The definitions, the
// sorting network and the combine rule are in pg_graph.h; here are the kernels and the C entries.
//
//   sorted()      count (a key (column << 32 | position in row) per entry, no-edge entries keyed behind every edge; valid entries
//                 per row) -> segmented sort of the rows' keys -> pg_exclusive_scan of the counts (caller) -> fill (column from
//                 the key, weight gathered by position).
//   transpose()   histogram (one integer atomicAdd per edge: exact in any order) -> pg_exclusive_scan (caller) -> scatter of the
//                 edges' 64-bit storage positions to t_indptr[c] + cursor[c]++ (a returning atomic: arrival order arbitrary)
//                 -> segmented sort of the columns' keys (the order is total, so the result is the same bits every run) ->
//                 emit (row by binary search in indptr, weight gathered by position).
//   symmetrize()  per row a rank-based merge of sorted(G)[r] and transpose(G)[r] into the workspace, heads of runs of equal
//                 column combine over their run and are kept or dropped by mode, count per row -> pg_exclusive_scan (caller)
//                 -> fill.
//
// The rate of RETURNING integer atomics that meet on one hub column has not been measured on this part (the guide's figures are
// for float adds without return); the scatter relies on them only for correctness.  tools/graph_ops_time.py times whole calls.
#include "pg_common.h"
#include "pg_graph.h"
#include "../../include/prograph_hip.h"

namespace {

typedef unsigned int u32;

struct BlockSync {
  __device__ void operator()() const { __syncthreads(); }
};

__device__ inline long long wave_sum_ll(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline bool is_edge(int c, long long ncols) { return c >= 0 && (long long)c < ncols; }

// ---------------------------------------------------------------- the segmented sort: every segment finds its tier itself
// tier 1: one wave per segment of at most PG_GRAPH_T1 keys, four segments per workgroup
__global__ __launch_bounds__(256) void pg_seg_sort_wave(const long long *__restrict__ segptr, long long nseg, pg_u64 *keys) {
  const int lane = threadIdx.x & 63;
  const long long seg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (seg >= nseg) return;
  const long long a = segptr[seg], n = segptr[seg + 1] - a;
  if (n < 2 || n > PG_GRAPH_T1) return;
  pg_u64 key = lane < n ? keys[a + lane] : PG_KEY_INF;
  const int P = (int)pg_pow2_ceil(n);
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int partner = (int)pg_bitonic_partner(lane, k, j);
      const pg_u64 theirs = __shfl(key, partner, 64);
      key = pg_wave_keep(key, theirs, lane, partner);
    }
  if (lane < n) keys[a + lane] = key;
}

// tiers 2 and 3: one workgroup per segment of more than PG_GRAPH_T1 keys
__global__ __launch_bounds__(256) void pg_seg_sort_block(const long long *__restrict__ segptr, pg_u64 *keys) {
  __shared__ pg_u64 chunk[PG_GRAPH_T2];
  const long long a = segptr[blockIdx.x], n = segptr[blockIdx.x + 1] - a;
  if (n <= PG_GRAPH_T1) return;
  pg_block_sort(keys + a, chunk, n, (long long)PG_GRAPH_T2, (int)threadIdx.x, 256, BlockSync());
}

int seg_sort(const long long *segptr, long long nseg, pg_u64 *keys, hipStream_t s) {
  pg_seg_sort_wave<<<dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, s>>>(segptr, nseg, keys);
  pg_seg_sort_block<<<dim3((unsigned)nseg), dim3(256), 0, s>>>(segptr, keys);
  return pg_launched("pg_seg_sort");
}

// ---------------------------------------------------------------- sorted()
__global__ __launch_bounds__(256) void pg_sort_rows_keys(const long long *__restrict__ indptr, const int *__restrict__ indices,
                                                         long long nrows, long long ncols, u32 *counts, pg_u64 *keys) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const long long a = indptr[row], b = indptr[row + 1];
  long long valid = 0;
  for (long long e = a + lane; e < b; e += 64) {
    const int c = indices[e];
    const bool ok = is_edge(c, ncols);
    keys[e] = ((ok ? (pg_u64)(u32)c : PG_NO_COLUMN) << 32) | (pg_u64)(u32)(e - a);
    valid += ok;
  }
  valid = wave_sum_ll(valid);
  if (lane == 0) counts[row] = (u32)valid;
}

__global__ __launch_bounds__(256) void pg_sort_rows_emit(const long long *__restrict__ indptr, const pg_u64 *__restrict__ keys,
                                                         const void *__restrict__ w, int eb, long long nrows,
                                                         const u32 *__restrict__ counts, const long long *__restrict__ out_indptr,
                                                         int *out_indices, void *out_w) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const long long a = indptr[row], o = out_indptr[row], n = counts[row];
  for (long long i = lane; i < n; i += 64) {
    const pg_u64 key = keys[a + i];
    out_indices[o + i] = (int)(key >> 32);
    pg_w_store(out_w, o + i, eb, pg_w_load(w, a + (long long)(key & 0xFFFFFFFFull), eb));
  }
}

// ---------------------------------------------------------------- transpose()
__global__ __launch_bounds__(256) void pg_histogram_kernel(const int *__restrict__ indices, long long nnz, long long ncols,
                                                           u32 *counts) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long long)gridDim.x * 256) {
    const int c = indices[e];
    if (is_edge(c, ncols)) atomicAdd(&counts[c], 1u);
  }
}

__global__ __launch_bounds__(256) void pg_transpose_scatter(const int *__restrict__ indices, long long nnz, long long ncols,
                                                            const long long *__restrict__ t_indptr, u32 *cursor, pg_u64 *keys) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (long long)gridDim.x * 256) {
    const int c = indices[e];
    if (is_edge(c, ncols)) keys[t_indptr[c] + (long long)atomicAdd(&cursor[c], 1u)] = (pg_u64)e;
  }
}

// one lane per edge of T: the key is the edge's storage position in G
__global__ __launch_bounds__(256) void pg_transpose_emit(const long long *__restrict__ indptr, const void *__restrict__ w, int eb,
                                                         long long nrows, long long row0, const long long *__restrict__ t_indptr,
                                                         long long ncols, const pg_u64 *__restrict__ keys, int *t_indices,
                                                         void *t_w) {
  const long long nnz_t = t_indptr[ncols];
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < nnz_t; s += (long long)gridDim.x * 256) {
    const long long e = (long long)keys[s];
    t_indices[s] = (int)(row0 + pg_row_of(indptr, nrows, e));
    pg_w_store(t_w, s, eb, pg_w_load(w, e, eb));
  }
}

// ---------------------------------------------------------------- symmetrize()
struct SymWs {                       // the workspace of M = nnz_a + nnz_t merged entries
  int *col;
  u32 *wbits;
  unsigned char *side, *keep;
};
SymWs sym_ws(void *workspace, long long m) {
  SymWs ws;
  ws.col = (int *)workspace;
  ws.wbits = (u32 *)workspace + m;
  ws.side = (unsigned char *)workspace + 8 * m;
  ws.keep = ws.side + m;
  return ws;
}

// pos(a_i) = i + lower_bound(T, a_i), pos(t_j) = j + upper_bound(A, t_j): of equal columns A's stand first
__global__ __launch_bounds__(256) void pg_sym_merge(const long long *__restrict__ a_indptr, const int *__restrict__ a_idx,
                                                    const void *__restrict__ a_w, const long long *__restrict__ t_indptr,
                                                    const int *__restrict__ t_idx, const void *__restrict__ t_w, int eb,
                                                    long long nrows, SymWs ws) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const long long a0 = a_indptr[row], na = a_indptr[row + 1] - a0, t0 = t_indptr[row], nt = t_indptr[row + 1] - t0, o = a0 + t0;
  for (long long i = lane; i < na; i += 64) {
    const int c = a_idx[a0 + i];
    const long long p = o + i + pg_lower_bound(t_idx + t0, nt, c);
    ws.col[p] = c; ws.wbits[p] = pg_w_load(a_w, a0 + i, eb); ws.side[p] = PG_SIDE_A;
  }
  for (long long j = lane; j < nt; j += 64) {
    const int c = t_idx[t0 + j];
    const long long p = o + j + pg_upper_bound(a_idx + a0, na, c);
    ws.col[p] = c; ws.wbits[p] = pg_w_load(t_w, t0 + j, eb); ws.side[p] = PG_SIDE_T;
  }
}

// the head of every run combines over its run (into its own wbits) and says whether the column is kept; other entries: 0
__global__ __launch_bounds__(256) void pg_sym_count(const long long *__restrict__ a_indptr, const long long *__restrict__ t_indptr,
                                                    int eb, int kind, int mode, int combine, long long nrows, SymWs ws,
                                                    u32 *counts) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const long long o = a_indptr[row] + t_indptr[row], len = a_indptr[row + 1] + t_indptr[row + 1] - o;
  long long kept = 0;
  for (long long p = lane; p < len; p += 64) {
    int keep = 0;
    if (p == 0 || ws.col[o + p - 1] != ws.col[o + p]) {
      int sides;
      const u32 w = pg_run_combine(ws.col + o, ws.wbits + o, ws.side + o, p, len, eb, kind, combine, &sides);
      keep = pg_run_kept(sides, mode);
      ws.wbits[o + p] = w;           // no other lane reads this word: it heads this lane's run
    }
    ws.keep[o + p] = (unsigned char)keep;
    kept += keep;
  }
  kept = wave_sum_ll(kept);
  if (lane == 0) counts[row] = (u32)kept;
}

__global__ __launch_bounds__(256) void pg_sym_fill(const long long *__restrict__ a_indptr, const long long *__restrict__ t_indptr,
                                                   int eb, long long nrows, SymWs ws, const long long *__restrict__ out_indptr,
                                                   int *out_idx, void *out_w) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const long long o = a_indptr[row] + t_indptr[row], len = a_indptr[row + 1] + t_indptr[row + 1] - o;
  long long at = out_indptr[row];
  for (long long p0 = 0; p0 < len; p0 += 64) {            // the whole wave takes every turn: the ballot needs all of it
    const long long p = p0 + lane;
    const bool keep = p < len && ws.keep[o + p];
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const long long q = at + __popcll(mask & ((1ull << lane) - 1ull));
      out_idx[q] = ws.col[o + p];
      pg_w_store(out_w, q, eb, ws.wbits[o + p]);
    }
    at += __popcll(mask);
  }
}

unsigned stride_grid(long long n) {
  const long long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > (1 << 20) ? (1 << 20) : g));
}
bool eb_ok(int eb) { return eb == 1 || eb == 2 || eb == 4; }
bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }
const long long kMaxI32 = 0x7fffffffll;

}  // namespace

extern "C" {

int64_t pg_csr_sort_workspace(int64_t nnz) { return nnz < 0 ? -1 : 8 * (nnz > 0 ? nnz : 1); }

int pg_csr_sort_rows_count(const int64_t *indptr, const int32_t *indices, int64_t nrows, int64_t nnz, int64_t ncols,
                           uint32_t *counts, void *workspace, int64_t workspace_bytes, void *stream) {
  if (!indptr || !indices || !counts || !workspace || nrows < 0 || nnz < 0 || ncols < 0 || nrows > kMaxI32 ||
      !aligned8(workspace))
    return pg_fail(PG_E_BADARG, "pg_csr_sort_rows_count: bad argument");
  if (workspace_bytes < pg_csr_sort_workspace(nnz)) return pg_fail(PG_E_BADARG, "pg_csr_sort_rows_count: the workspace is too small");
  if (nrows == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  pg_sort_rows_keys<<<dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, s>>>((const long long *)indptr, indices, nrows, ncols,
                                                                           counts, (pg_u64 *)workspace);
  if (nnz == 0) return pg_launched("pg_sort_rows_keys");
  return seg_sort((const long long *)indptr, nrows, (pg_u64 *)workspace, s);
}

int pg_csr_sort_rows_fill(const int64_t *indptr, const void *weights, int elem_bytes, int64_t nrows, int64_t nnz,
                          const uint32_t *counts, const int64_t *out_indptr, int32_t *out_indices, void *out_weights,
                          const void *workspace, int64_t workspace_bytes, void *stream) {
  if (!indptr || !weights || !counts || !out_indptr || !out_indices || !out_weights || !workspace || nrows < 0 || nnz < 0 ||
      nrows > kMaxI32 || !eb_ok(elem_bytes) || !aligned8(workspace))
    return pg_fail(PG_E_BADARG, "pg_csr_sort_rows_fill: bad argument");
  if (workspace_bytes < pg_csr_sort_workspace(nnz)) return pg_fail(PG_E_BADARG, "pg_csr_sort_rows_fill: the workspace is too small");
  if (nrows == 0 || nnz == 0) return 0;
  pg_sort_rows_emit<<<dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      (const long long *)indptr, (const pg_u64 *)workspace, weights, elem_bytes, nrows, counts, (const long long *)out_indptr,
      out_indices, out_weights);
  return pg_launched("pg_sort_rows_emit");
}

int pg_csr_histogram(const int32_t *indices, int64_t nnz, int64_t ncols, uint32_t *counts, void *stream) {
  if (!indices || !counts || nnz < 0 || ncols < 0 || ncols > kMaxI32) return pg_fail(PG_E_BADARG, "pg_csr_histogram: bad argument");
  if (ncols == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = (int)hipMemsetAsync(counts, 0, (size_t)ncols * sizeof(u32), s)) return pg_launched(rc, "pg_csr_histogram");
  if (nnz == 0) return 0;
  pg_histogram_kernel<<<dim3(stride_grid(nnz)), dim3(256), 0, s>>>(indices, nnz, ncols, counts);
  return pg_launched("pg_histogram_kernel");
}

int64_t pg_csr_transpose_workspace(int64_t nnz, int64_t ncols) {
  return nnz < 0 || ncols < 0 ? -1 : 8 * (nnz > 0 ? nnz : 1) + 4 * (ncols > 0 ? ncols : 1);
}

int pg_csr_transpose(const int64_t *indptr, const int32_t *indices, const void *weights, int elem_bytes, int64_t nrows,
                     int64_t nnz, int64_t ncols, int64_t row0, const int64_t *t_indptr, int32_t *t_indices, void *t_weights,
                     void *workspace, int64_t workspace_bytes, void *stream) {
  if (!indptr || !indices || !weights || !t_indptr || !t_indices || !t_weights || !workspace || nrows < 0 || nnz < 0 ||
      ncols < 0 || row0 < 0 || ncols > kMaxI32 || row0 + nrows > kMaxI32 || !eb_ok(elem_bytes) || !aligned8(workspace))
    return pg_fail(PG_E_BADARG, "pg_csr_transpose: bad argument");
  if (workspace_bytes < pg_csr_transpose_workspace(nnz, ncols)) return pg_fail(PG_E_BADARG, "pg_csr_transpose: the workspace is too small");
  if (nrows == 0 || nnz == 0 || ncols == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  pg_u64 *keys = (pg_u64 *)workspace;
  u32 *cursor = (u32 *)(keys + nnz);
  if (int rc = (int)hipMemsetAsync(cursor, 0, (size_t)ncols * sizeof(u32), s)) return pg_launched(rc, "pg_csr_transpose");
  pg_transpose_scatter<<<dim3(stride_grid(nnz)), dim3(256), 0, s>>>(indices, nnz, ncols, (const long long *)t_indptr, cursor, keys);
  if (int rc = seg_sort((const long long *)t_indptr, ncols, keys, s)) return rc;
  pg_transpose_emit<<<dim3(stride_grid(nnz)), dim3(256), 0, s>>>((const long long *)indptr, weights, elem_bytes, nrows, row0,
                                                                  (const long long *)t_indptr, ncols, keys, t_indices, t_weights);
  return pg_launched("pg_transpose_emit");
}

int64_t pg_csr_symmetrize_workspace(int64_t nnz_a, int64_t nnz_t) {
  return nnz_a < 0 || nnz_t < 0 ? -1 : 10 * (nnz_a + nnz_t > 0 ? nnz_a + nnz_t : 1);
}

int pg_csr_symmetrize_count(const int64_t *a_indptr, const int32_t *a_indices, const void *a_weights, int64_t nnz_a,
                            const int64_t *t_indptr, const int32_t *t_indices, const void *t_weights, int64_t nnz_t,
                            int elem_bytes, int kind, int mode, int combine, int64_t nrows, uint32_t *counts, void *workspace,
                            int64_t workspace_bytes, void *stream) {
  if (!a_indptr || !a_indices || !a_weights || !t_indptr || !t_indices || !t_weights || !counts || !workspace || nrows < 0 ||
      nnz_a < 0 || nnz_t < 0 || nrows > kMaxI32 || !aligned8(workspace))
    return pg_fail(PG_E_BADARG, "pg_csr_symmetrize_count: bad argument");
  if (!pg_w_kind_ok(elem_bytes, kind)) return pg_fail(PG_E_BADARG, "pg_csr_symmetrize_count: elem_bytes 1, 2 or 4 of kind 0 (unsigned), 1 (signed) or 2 (float, not 1 byte)");
  if ((mode != PG_SYM_UNION && mode != PG_SYM_MUTUAL) || (combine != PG_COMBINE_MIN && combine != PG_COMBINE_MAX))
    return pg_fail(PG_E_BADARG, "pg_csr_symmetrize_count: mode 0 (union) or 1 (mutual), combine 0 (min) or 1 (max)");
  if (workspace_bytes < pg_csr_symmetrize_workspace(nnz_a, nnz_t)) return pg_fail(PG_E_BADARG, "pg_csr_symmetrize_count: the workspace is too small");
  if (nrows == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const SymWs ws = sym_ws(workspace, nnz_a + nnz_t);
  const dim3 grid((unsigned)((nrows + 3) / 4));
  pg_sym_merge<<<grid, dim3(256), 0, s>>>((const long long *)a_indptr, a_indices, a_weights, (const long long *)t_indptr, t_indices,
                                          t_weights, elem_bytes, nrows, ws);
  pg_sym_count<<<grid, dim3(256), 0, s>>>((const long long *)a_indptr, (const long long *)t_indptr, elem_bytes, kind, mode, combine,
                                          nrows, ws, counts);
  return pg_launched("pg_sym_count");
}

int pg_csr_symmetrize_fill(const int64_t *a_indptr, int64_t nnz_a, const int64_t *t_indptr, int64_t nnz_t, int elem_bytes,
                           int64_t nrows, const int64_t *out_indptr, int32_t *out_indices, void *out_weights,
                           const void *workspace, int64_t workspace_bytes, void *stream) {
  if (!a_indptr || !t_indptr || !out_indptr || !out_indices || !out_weights || !workspace || nrows < 0 || nnz_a < 0 || nnz_t < 0 ||
      nrows > kMaxI32 || !eb_ok(elem_bytes) || !aligned8(workspace))
    return pg_fail(PG_E_BADARG, "pg_csr_symmetrize_fill: bad argument");
  if (workspace_bytes < pg_csr_symmetrize_workspace(nnz_a, nnz_t)) return pg_fail(PG_E_BADARG, "pg_csr_symmetrize_fill: the workspace is too small");
  if (nrows == 0 || nnz_a + nnz_t == 0) return 0;
  pg_sym_fill<<<dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      (const long long *)a_indptr, (const long long *)t_indptr, elem_bytes, nrows, sym_ws(const_cast<void *>(workspace), nnz_a + nnz_t),
      (const long long *)out_indptr, out_indices, out_weights);
  return pg_launched("pg_sym_fill");
}

}  // extern "C"
