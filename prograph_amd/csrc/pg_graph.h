// Undirected device graphs: the pieces of pg_graph.hip that run on the host as well - the sorting network's
// schedule, the merge ranks, the combine rule.  tests/capi_graph compiles this file alone for the CPU.
//
// DEFINITIONS.  A graph G is a CSR with nrows rows, ncols columns and row0 (row r is node row0 + r).  An entry whose column is
// outside 0..ncols-1 is no edge (-1, the empty kNN slot, among them; the rule of pg_csr_row_stats): it is never read through and
// nothing is written for it.  "Storage order" is the order of the entries in `indices`.
//   sorted(G)      the same rows, each row's edges ascending by column; equal columns keep their storage order (stable); weights
//                  travel with their entries, bits untouched; no-edge entries are dropped.
//   transpose(G)   T with T.nrows = G.ncols, T.ncols = G.row0 + G.nrows, T.row0 = 0: row c of T lists (G.row0 + r, w) for every
//                  edge (r, c, w) of G in G's storage order - so its columns are ascending and duplicates keep their order.
//                  Bitwise reproducible: what the atomics scatter is the edge's storage position, a key the sort orders totally.
//   symmetrize(G)  for row0 == 0 and nrows == ncols, S with rows ascending by column and each column at most once per row;
//                  union: (r, c) in S iff (r, c) or (c, r) is an edge of G; mutual: iff both are.  S[r, c] = combine (min | max)
//                  over the weights of ALL occurrences of (r, c) and (c, r) in G; a self-loop is its own reverse.
//                  Integers compare as integers, floats as floats; so that S equals transpose(S) bit for bit the winner of two
//                  weights is a function of the unordered pair (pg_w_pick): a NaN loses to a number under min and under max,
//                  of two NaNs and of two equal floats (-0 and +0) the smaller bit pattern wins (+0 over -0).
//
// THE SORT.  Segments of distinct 64-bit keys, ascending.  The network is the bitonic sorter in its all-ascending form: merge stage
// k = 2, 4, .. P (P = the power of two at or above the length) opens with the step that pairs i with its mirror in its block of k
// (i ^ (k - 1)) and goes on with the steps j = k/4 .. 1 that pair i with i ^ j.  Every compare-exchange puts the smaller key at the
// lower index - there is no direction bit -, so an index at or past the length, which stands for a key of +infinity, never moves:
// a pair whose upper index is past the length is skipped (virtual padding; nothing is read or written there).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PG_HD __host__ __device__
#else
#define PG_HD
#endif

typedef unsigned long long pg_u64;

// Tier limits of the segmented sort.  UNMEASURED tuning values (profiles/graph_ops.txt records the time per tier):
#define PG_GRAPH_T1 64      // a segment of up to this many keys: one wave's registers, the network over __shfl_xor
#define PG_GRAPH_T2 4096    // up to this many: the LDS of one 256-lane workgroup (8 bytes a key: 32 KB); beyond: the same
//                             workgroup over global memory, with every run of steps that stays inside 4096 keys done in LDS
#define PG_KEY_INF (~0ull)  // the key of a lane without one (tier 1); above every key either use forms
#define PG_NO_COLUMN 0xFFFFFFFFull   // sorted(): the column field of a no-edge entry's key - it sorts behind every edge of its row

#define PG_W_UNSIGNED 0
#define PG_W_SIGNED 1
#define PG_W_FLOAT 2
#define PG_SYM_UNION 0
#define PG_SYM_MUTUAL 1
#define PG_COMBINE_MIN 0
#define PG_COMBINE_MAX 1
#define PG_SIDE_A 1         // the entry comes from sorted(G)'s row
#define PG_SIDE_T 2         // from transpose(G)'s row

PG_HD inline long long pg_pow2_ceil(long long n) {
  long long p = 1;
  while (p < n) p <<= 1;
  return p;
}

// partner of index i in step j of merge stage k (j = k/2, k/4, .. 1)
PG_HD inline long long pg_bitonic_partner(long long i, long long k, long long j) { return j * 2 == k ? i ^ (k - 1) : i ^ j; }

// the t-th pair of step (k, j): lo < hi, t in 0 .. P/2 - 1; the pairs of an aligned block of 2j indices are consecutive in t
PG_HD inline void pg_bitonic_pair(long long t, long long k, long long j, long long *lo, long long *hi) {
  const long long i = (t / j) * (2 * j) + t % j;
  *lo = i;
  *hi = pg_bitonic_partner(i, k, j);
}

PG_HD inline void pg_cmpx(pg_u64 *a, pg_u64 *b) {
  const pg_u64 x = *a, y = *b;
  if (x > y) { *a = y; *b = x; }
}

// tier 1: what lane `lane` keeps of its own key and its partner's
PG_HD inline pg_u64 pg_wave_keep(pg_u64 mine, pg_u64 theirs, int lane, int partner) {
  return (lane < partner) == (mine < theirs) ? mine : theirs;
}

// steps (k, j), (k, j/2), .. (k, 1) on the chunk [base, base + C) of a segment of n keys whose keys stand in buf[0 .. C);
// C a power of two, base a multiple of C, 2j <= C.  `lane` of `lanes` (one workgroup; the host test runs it with 1 of 1).
template <class Sync>
PG_HD inline void pg_steps_in_chunk(pg_u64 *buf, long long base, long long C, long long n, long long k, long long j, int lane,
                                    int lanes, Sync sync) {
  for (; j > 0; j >>= 1) {
    for (long long t = lane; t < C / 2; t += lanes) {
      long long lo, hi;
      pg_bitonic_pair(base / 2 + t, k, j, &lo, &hi);
      if (hi < n) pg_cmpx(&buf[lo - base], &buf[hi - base]);
    }
    sync();
  }
}

// Tiers 2 and 3: one workgroup sorts g[0 .. n) ascending, any n.  `chunk`: room for min(P, T2) keys (LDS on the device), T2 a power
// of two.  n <= T2: one load, the whole network in the chunk, one store.  Beyond: every chunk of T2 keys is sorted in the chunk
// (stages 2 .. T2), then every stage k = 2 T2 .. P runs its steps j >= T2 on global memory and its steps j < T2 chunk by chunk.
template <class Sync>
PG_HD inline void pg_block_sort(pg_u64 *g, pg_u64 *chunk, long long n, long long T2, int lane, int lanes, Sync sync) {
  if (n < 2) return;
  const long long P = pg_pow2_ceil(n), C = P < T2 ? P : T2;
  for (long long k0 = C; k0 <= P; k0 <<= 1) {             // k0 = C: stages 2 .. C; then stage k0 itself
    if (k0 > C) {
      for (long long j = k0 / 2; j >= C; j >>= 1) {
        for (long long t = lane; t < P / 2; t += lanes) {
          long long lo, hi;
          pg_bitonic_pair(t, k0, j, &lo, &hi);
          if (hi < n) pg_cmpx(&g[lo], &g[hi]);
        }
        sync();
      }
    }
    for (long long base = 0; base < n; base += C) {
      const long long cnt = n - base < C ? n - base : C;
      for (long long i = lane; i < cnt; i += lanes) chunk[i] = g[base + i];
      sync();
      if (k0 == C) {
        for (long long k = 2; k <= C; k <<= 1) pg_steps_in_chunk(chunk, base, C, n, k, k / 2, lane, lanes, sync);
      } else {
        pg_steps_in_chunk(chunk, base, C, n, k0, C / 2, lane, lanes, sync);
      }
      for (long long i = lane; i < cnt; i += lanes) g[base + i] = chunk[i];
      sync();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// merge ranks: a[0 .. n) ascending
PG_HD inline long long pg_lower_bound(const int *a, long long n, int v) {     // entries below v
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
PG_HD inline long long pg_upper_bound(const int *a, long long n, int v) {     // entries at or below v
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (a[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the row r with indptr[r] <= e < indptr[r + 1] (empty rows in between are passed over); e in 0 .. indptr[nrows] - 1
PG_HD inline long long pg_row_of(const long long *indptr, long long nrows, long long e) {
  long long lo = 0, hi = nrows;                                               // the last r with indptr[r] <= e
  while (hi - lo > 1) {
    const long long mid = lo + (hi - lo) / 2;
    if (indptr[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------------------------
// weights as bits: 1, 2 or 4 bytes, zero-extended to 32
PG_HD inline unsigned pg_w_load(const void *w, long long e, int elem_bytes) {
  if (elem_bytes == 1) return ((const unsigned char *)w)[e];
  if (elem_bytes == 2) return ((const unsigned short *)w)[e];
  return ((const unsigned *)w)[e];
}
PG_HD inline void pg_w_store(void *w, long long e, int elem_bytes, unsigned bits) {
  if (elem_bytes == 1) ((unsigned char *)w)[e] = (unsigned char)bits;
  else if (elem_bytes == 2) ((unsigned short *)w)[e] = (unsigned short)bits;
  else ((unsigned *)w)[e] = bits;
}

// binary16 bits -> the float of the same value (exact; NaNs stay NaNs)
PG_HD inline float pg_half_bits_to_float(unsigned h) {
  const unsigned sign = (h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 0x3FFu;
  unsigned f;
  if (ex == 31u) f = sign | 0x7F800000u | (man << 13);
  else if (ex) f = sign | ((ex + 112u) << 23) | (man << 13);
  else if (!man) f = sign;
  else {                                                  // subnormal: man * 2^-24
    int e = 0;
    unsigned m = man;
    while (!(m & 0x400u)) { m <<= 1; ++e; }
    f = sign | ((unsigned)(113 - e) << 23) | ((m & 0x3FFu) << 13);
  }
  union { unsigned u; float v; } c;
  c.u = f;
  return c.v;
}

PG_HD inline int pg_w_kind_ok(int elem_bytes, int kind) {
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return 0;
  if (kind == PG_W_FLOAT) return elem_bytes != 1;
  return kind == PG_W_UNSIGNED || kind == PG_W_SIGNED;
}

// The winner of two weights under min / max: a function of the unordered pair {a, b}, and the minimum of a total order on the bit
// patterns, so that a combine over any number of weights does not depend on their order.
PG_HD inline unsigned pg_w_pick(unsigned a, unsigned b, int elem_bytes, int kind, int combine) {
  const unsigned small = a < b ? a : b;                   // the tie rule: the smaller bit pattern
  int lt, gt;                                             // a below / above b in value
  if (kind == PG_W_FLOAT) {
    union { unsigned u; float v; } ca, cb;
    ca.u = a; cb.u = b;
    const float fa = elem_bytes == 2 ? pg_half_bits_to_float(a) : ca.v, fb = elem_bytes == 2 ? pg_half_bits_to_float(b) : cb.v;
    const int na = fa != fa, nb = fb != fb;
    if (na || nb) return na && nb ? small : (na ? b : a); // a NaN loses to a number whatever the combine
    lt = fa < fb; gt = fa > fb;
  } else if (kind == PG_W_SIGNED) {
    const int sh = 32 - 8 * elem_bytes;
    const int sa = (int)(a << sh) >> sh, sb = (int)(b << sh) >> sh;
    lt = sa < sb; gt = sa > sb;
  } else {
    lt = a < b; gt = a > b;
  }
  if (!lt && !gt) return small;
  return (combine == PG_COMBINE_MIN) == (lt != 0) ? a : b;
}

// The run of equal column that starts at p in a merged row col[0 .. len) (side: PG_SIDE_A | PG_SIDE_T per entry, wbits: the
// weights' bits): the combined weight, the sides that hold the column in *sides.
PG_HD inline unsigned pg_run_combine(const int *col, const unsigned *wbits, const unsigned char *side, long long p, long long len,
                                     int elem_bytes, int kind, int combine, int *sides) {
  unsigned w = wbits[p];
  int s = side[p];
  for (long long q = p + 1; q < len && col[q] == col[p]; ++q) {
    w = pg_w_pick(w, wbits[q], elem_bytes, kind, combine);
    s |= side[q];
  }
  *sides = s;
  return w;
}
PG_HD inline int pg_run_kept(int sides, int mode) { return mode == PG_SYM_UNION || sides == (PG_SIDE_A | PG_SIDE_T); }
