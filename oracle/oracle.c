/*
 * ORACLE (C leg) — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Plain C restatement of the reference's hot path (acmater/prograph; citations into
 * /root/reference) for sizes where the Python oracle (oracle/prograph_oracle.py) is too slow.
 * Pinned: tests/test_oracle.py checks every function here against the Python oracle, which is
 * itself pinned to golden vectors generated from the real reference.  Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library.
 *
 *   orc_hamming   d[m][n] = #{j : Y[m][j] != X[n][j]}            prograph/distance/hamming.py:34
 *   orc_eps       (comp(d,eps) & (d>0)) per row, columns ascending prograph/prograph.py:731-753
 *   orc_knn       stable ascending sort by distance, ranks 1..k    prograph/prograph.py:756-764
 *   orc_synth     the deterministic generator of prograph_amd/synth.py
 *   orc_align_trace  the canonical alignment of DESIGN.md §4.20 with whole tables (build defined, below)
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static inline int ham(const uint8_t *a, const uint8_t *b, int l) {
  int d = 0;
  for (int j = 0; j < l; ++j) d += a[j] != b[j];
  return d;
}

void orc_hamming(const uint8_t *X, int64_t n, const uint8_t *Y, int64_t m, int l, int64_t *out) {
#pragma omp parallel for schedule(static)
  for (int64_t r = 0; r < m; ++r)
    for (int64_t c = 0; c < n; ++c) out[r * n + c] = ham(Y + r * l, X + c * l, l);
}

static inline int cmp_ok(int cmp, double d, double eps) {
  switch (cmp) {
    case 0: return d <= eps;
    case 1: return d < eps;
    case 2: return d == eps;
    case 3: return d >= eps;
    default: return d > eps;
  }
}

/* pass 1 (indices == NULL): counts[r]; pass 2: fill indices/weights at indptr[r] */
void orc_eps(const uint8_t *T, int64_t n, int l, int64_t row0, int64_t nrows, int cmp, double eps,
             int64_t *counts, const int64_t *indptr, int32_t *indices, uint8_t *weights) {
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t r = 0; r < nrows; ++r) {
    const uint8_t *a = T + (row0 + r) * l;
    int64_t k = 0, base = indices ? indptr[r] : 0;
    for (int64_t c = 0; c < n; ++c) {
      int d = ham(a, T + c * l, l);
      if (d > 0 && cmp_ok(cmp, (double)d, eps)) {
        if (indices) { indices[base + k] = (int32_t)c; weights[base + k] = (uint8_t)d; }
        ++k;
      }
    }
    if (!indices) counts[r] = k;
  }
}

/* canonical kNN: k+1 smallest (d, column), rank 0 dropped; missing ranks -> -1 / 255 */
void orc_knn(const uint8_t *T, int64_t n, int l, int64_t row0, int64_t nrows, int k, int32_t *idx, uint8_t *dist) {
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t r = 0; r < nrows; ++r) {
    const uint8_t *a = T + (row0 + r) * l;
    int64_t best[1026];                      /* k <= 1024 */
    int nb = 0;
    for (int64_t c = 0; c < n; ++c) {
      int64_t key = ((int64_t)ham(a, T + c * l, l) << 32) | c;
      if (nb == k + 1 && key >= best[nb - 1]) continue;
      int p = nb < k + 1 ? nb++ : nb - 1;
      while (p > 0 && best[p - 1] > key) { best[p] = best[p - 1]; --p; }
      best[p] = key;
    }
    for (int j = 0; j < k; ++j) {
      if (j + 1 < nb) { idx[r * k + j] = (int32_t)(best[j + 1] & 0xffffffff); dist[r * k + j] = (uint8_t)(best[j + 1] >> 32); }
      else { idx[r * k + j] = -1; dist[r * k + j] = 255; }
    }
  }
}

/* ---------------------------------------------------------------------------------------
 * FAST LEG of orc_eps / orc_knn for full-size checks (N = 200 000: 4e10 pairs).  The same definitions -
 * d = number of differing token bytes; (comp(d, eps) & d > 0), columns ascending; the k + 1 smallest
 * (d, column) keys, rank 0 dropped - with the byte compare done 32 bytes at a time (AVX2 vpcmpeqb +
 * movemask + popcount; plain 8-byte words where AVX2 is missing).  Pinned: tests/test_oracle.py checks it
 * against the scalar functions above on ragged lengths.
 * ------------------------------------------------------------------------------------- */
#if defined(__x86_64__)
#include <immintrin.h>
__attribute__((target("avx2,popcnt"))) static int ham_avx2(const uint8_t *a, const uint8_t *b, int l) {
  int eq = 0, j = 0;
  for (; j + 32 <= l; j += 32) {
    const __m256i x = _mm256_loadu_si256((const __m256i *)(a + j)), y = _mm256_loadu_si256((const __m256i *)(b + j));
    eq += __builtin_popcount((unsigned)_mm256_movemask_epi8(_mm256_cmpeq_epi8(x, y)));
  }
  int d = j - eq;
  for (; j < l; ++j) d += a[j] != b[j];
  return d;
}
#endif
static int ham_words(const uint8_t *a, const uint8_t *b, int l) {
  int d = 0, j = 0;
  for (; j + 8 <= l; j += 8) {
    uint64_t x, y;
    memcpy(&x, a + j, 8); memcpy(&y, b + j, 8);
    x ^= y;
    x |= x >> 4; x |= x >> 2; x |= x >> 1;                /* bit 0 of every byte: the byte differs */
    d += __builtin_popcountll(x & 0x0101010101010101ULL);
  }
  for (; j < l; ++j) d += a[j] != b[j];
  return d;
}
typedef int (*ham_fn)(const uint8_t *, const uint8_t *, int);
static ham_fn pick_ham(void) {
#if defined(__x86_64__)
  if (__builtin_cpu_supports("avx2") && __builtin_cpu_supports("popcnt")) return ham_avx2;
#endif
  return ham_words;
}

void orc_eps_fast(const uint8_t *T, int64_t n, int l, int64_t row0, int64_t nrows, int cmp, double eps,
                  int64_t *counts, const int64_t *indptr, int32_t *indices, uint8_t *weights) {
  const ham_fn hf = pick_ham();
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t r = 0; r < nrows; ++r) {
    const uint8_t *a = T + (row0 + r) * l;
    int64_t k = 0, base = indices ? indptr[r] : 0;
    for (int64_t c = 0; c < n; ++c) {
      const int d = hf(a, T + c * l, l);
      if (d > 0 && cmp_ok(cmp, (double)d, eps)) {
        if (indices) { indices[base + k] = (int32_t)c; weights[base + k] = (uint8_t)d; }
        ++k;
      }
    }
    if (!indices) counts[r] = k;
  }
}

void orc_knn_fast(const uint8_t *T, int64_t n, int l, int64_t row0, int64_t nrows, int k, int32_t *idx, uint8_t *dist) {
  const ham_fn hf = pick_ham();
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t r = 0; r < nrows; ++r) {
    const uint8_t *a = T + (row0 + r) * l;
    int64_t best[1026];                      /* k <= 1024 */
    int nb = 0;
    for (int64_t c = 0; c < n; ++c) {
      const int64_t key = ((int64_t)hf(a, T + c * l, l) << 32) | c;
      if (nb == k + 1 && key >= best[nb - 1]) continue;
      int p = nb < k + 1 ? nb++ : nb - 1;
      while (p > 0 && best[p - 1] > key) { best[p] = best[p - 1]; --p; }
      best[p] = key;
    }
    for (int j = 0; j < k; ++j) {
      if (j + 1 < nb) { idx[r * k + j] = (int32_t)(best[j + 1] & 0xffffffff); dist[r * k + j] = (uint8_t)(best[j + 1] >> 32); }
      else { idx[r * k + j] = -1; dist[r * k + j] = 255; }
    }
  }
}

static inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}
static inline uint64_t hh(uint64_t seed, uint64_t stream, uint64_t i) {
  return mix64(seed + 0x9E3779B97F4A7C15ULL * (4 * i + stream + 1));
}

void orc_synth(int64_t n, int l, uint64_t seed, int64_t members, uint8_t *out) {
  int64_t nc = n / members;
  if (nc < 1) nc = 1;
  for (int64_t i = 0; i < n; ++i) {
    int64_t c = i % nc;
    uint8_t *row = out + i * l;
    for (int j = 0; j < l; ++j) row[j] = (uint8_t)(1 + hh(seed, 0, (uint64_t)(c * l + j)) % 20);
    int m = 1 + (int)(hh(seed, 1, (uint64_t)i) % 3);
    /* positions and steps are drawn from the UNMUTATED row index stream; substitutions apply in
       order t = 0,1,2 and each reads the token as left by the previous ones */
    for (int t = 0; t < m; ++t) {
      int pos = (int)(hh(seed, 2, (uint64_t)(8 * i + t)) % (uint64_t)l);
      int step = (int)(hh(seed, 3, (uint64_t)(8 * i + t)) % 19);
      row[pos] = (uint8_t)(1 + ((row[pos] - 1 + 1 + step) % 20));
    }
  }
}

/* ---------------------------------------------------------------------------------------
 * Banded Levenshtein kNN — BUILD DEFINED (no reference counterpart; parity unpinned).
 * d(a,b) = min(edit_distance(a,b), band+1) on the non-zero prefixes; plain Wagner–Fischer
 * restricted to |i-j| <= band (exact whenever the true distance is <= band, > band otherwise),
 * then the canonical (d, column) order, rank 0 dropped, ranks 1..k.
 * ------------------------------------------------------------------------------------- */
static int seq_len(const uint8_t *a, int l) {
  int n = 0;
  while (n < l && a[n] != 0) ++n;
  return n;
}

int orc_lev_pair(const uint8_t *a, int la, const uint8_t *b, int lb, int band) {
  const int cap = band + 1, INF = 1 << 20;
  if (la - lb > band || lb - la > band) return cap;
  int prev[130], cur[130];
  for (int j = 0; j <= lb; ++j) prev[j] = j <= band ? j : INF;
  for (int i = 1; i <= la; ++i) {
    int lo = i - band < 0 ? 0 : i - band, hi = i + band > lb ? lb : i + band;
    for (int j = 0; j <= lb; ++j) cur[j] = INF;
    if (lo == 0) cur[0] = i;
    for (int j = lo < 1 ? 1 : lo; j <= hi; ++j) {
      int v = prev[j - 1] + (a[i - 1] != b[j - 1]);
      if (prev[j] + 1 < v) v = prev[j] + 1;
      if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
      cur[j] = v;
    }
    memcpy(prev, cur, sizeof(int) * (size_t)(lb + 1));
  }
  return prev[lb] < cap ? prev[lb] : cap;
}

void orc_lev_knn(const uint8_t *T, int64_t n, int l, int64_t row0, int64_t nrows, int band, int k,
                 int32_t *idx, uint8_t *dist) {
  int *lens = (int *)malloc(sizeof(int) * (size_t)n);
  for (int64_t i = 0; i < n; ++i) lens[i] = seq_len(T + i * l, l);
#pragma omp parallel for schedule(dynamic, 8)
  for (int64_t r = 0; r < nrows; ++r) {
    const uint8_t *a = T + (row0 + r) * l;
    int64_t best[65];
    int nb = 0;
    for (int64_t c = 0; c < n; ++c) {
      int64_t key = ((int64_t)orc_lev_pair(a, lens[row0 + r], T + c * l, lens[c], band) << 32) | c;
      if (nb == k + 1 && key >= best[nb - 1]) continue;
      int p = nb < k + 1 ? nb++ : nb - 1;
      while (p > 0 && best[p - 1] > key) { best[p] = best[p - 1]; --p; }
      best[p] = key;
    }
    for (int j = 0; j < k; ++j) {
      if (j + 1 < nb) { idx[r * k + j] = (int32_t)(best[j + 1] & 0xffffffff); dist[r * k + j] = (uint8_t)(best[j + 1] >> 32); }
      else { idx[r * k + j] = -1; dist[r * k + j] = 255; }
    }
  }
  free(lens);
}

/* ---------------------------------------------------------------------------------------
 * Unbanded Levenshtein matrix — BUILD DEFINED (no reference counterpart).
 * out[r * n + c] = edit distance (unit costs) of the non-zero prefix of Y row r against the
 * non-zero prefix of X row c: the plain Wagner–Fischer table kept as two rows.  X is (n, lx),
 * Y is (m, ly), zero right-padded, lx and ly up to 2048.  out is int32 (out_bytes 4) or int64 (8).
 * Pinned against the numpy references in tests/test_levenshtein_every_length_cpu.py.
 * ------------------------------------------------------------------------------------- */
#define ORC_LEV_MATRIX_MAX 2048
void orc_lev_matrix(const uint8_t *X, int64_t n, int lx, const uint8_t *Y, int64_t m, int ly, void *out, int out_bytes) {
  if (lx > ORC_LEV_MATRIX_MAX || ly > ORC_LEV_MATRIX_MAX || lx < 0 || ly < 0) return;
  int *xlens = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
  for (int64_t c = 0; c < n; ++c) xlens[c] = seq_len(X + c * lx, lx);
#pragma omp parallel for schedule(dynamic, 1)
  for (int64_t r = 0; r < m; ++r) {
    const uint8_t *a = Y + r * ly;
    const int la = seq_len(a, ly);
    int rowa[ORC_LEV_MATRIX_MAX + 1], rowb[ORC_LEV_MATRIX_MAX + 1];
    for (int64_t c = 0; c < n; ++c) {
      const uint8_t *b = X + c * lx;
      const int lb = xlens[c];
      int *prev = rowa, *cur = rowb;
      for (int j = 0; j <= lb; ++j) prev[j] = j;
      for (int i = 1; i <= la; ++i) {
        cur[0] = i;
        for (int j = 1; j <= lb; ++j) {
          int v = prev[j - 1] + (a[i - 1] != b[j - 1]);
          if (prev[j] + 1 < v) v = prev[j] + 1;
          if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
          cur[j] = v;
        }
        int *t = prev; prev = cur; cur = t;
      }
      if (out_bytes == 8) ((int64_t *)out)[r * n + c] = prev[lb];
      else ((int32_t *)out)[r * n + c] = prev[lb];
    }
  }
  free(xlens);
}

/* ---------------------------------------------------------------------------------------
 * Canonical alignment of a list of pairs — BUILD DEFINED (no reference counterpart).
 * The yardstick of tests/test_alignment_trace_lengths_*.py: tests/trace_testdata.definition (fit:
 * tests/fit_testdata.canonical) restated in C, to which tests/test_alignment_trace_lengths_cpu.py pins it.  Per pair the
 * three tables H, E, F are kept WHOLE as int64, the global distance minimising over its cost table and the three scores
 * maximising; the end cell is found by a scan of the finished table in the canonical order (by i, then j; only a
 * larger value replaces); the walk back compares table entries.  Nothing of the kernels' shape is here: no direction
 * bits, no negated table, no running maximum, no strips.
 *
 * X (n, xw), Y (m, yw): uint8 rows, zero right-padded, a sequence is a row without its trailing zeros (an interior zero
 * is symbol 0).  T is (A, A) int64, read as T[x symbol][y symbol].  mode 0 global distance, 1 local, 2 semi-global,
 * 3 fit (all of y within x).  head is int32 (P, 8) = score, x_begin, x_end, y_begin, y_end, n_ops, identities, 0;
 * ops uint8 (P, ldo): 1 pair, 2 x symbol unaligned, 3 y symbol unaligned, 0 from n_ops on.
 * Returns 0, or 1 an index outside its operand, 2 a symbol outside the table, 3 a pair of more than
 * ORC_TRACE_MAX_CELLS cells, 4 ldo below len x + len y, 5 a bad argument, 6 no memory; nothing is promised of head
 * and ops then.
 * ------------------------------------------------------------------------------------- */
#define ORC_TRACE_MAX_CELLS (1 << 19)
#define ORC_TRACE_NONE ((int64_t)1 << 40)

static int row_len(const uint8_t *a, int w) {
  int n = w;
  while (n > 0 && a[n - 1] == 0) --n;
  return n;
}

static inline int64_t orc_better(int mn, int64_t a, int64_t b) { return mn ? (a < b ? a : b) : (a > b ? a : b); }

static void orc_trace_pair(int mode, const int64_t *T, int A, int64_t e, int64_t o, const uint8_t *x, int lx, const uint8_t *y,
                           int ly, int64_t *H, int64_t *E, int64_t *F, int32_t *head, uint8_t *ops, int64_t ldo) {
  const int mn = mode == 0, W = ly + 1;
  const int64_t none = mn ? ORC_TRACE_NONE : -ORC_TRACE_NONE, oe = mn ? o + e : -(o + e), ee = mn ? e : -e;
#define AT(M, i, j) M[(int64_t)(i) * W + (j)]
  for (int i = 0; i <= lx; ++i)
    for (int j = 0; j <= ly; ++j) {
      AT(H, i, j) = 0;
      AT(E, i, j) = none;
      AT(F, i, j) = none;
    }
  if (mode == 0) {
    for (int j = 1; j <= ly; ++j) AT(H, 0, j) = o + j * e;
    for (int i = 1; i <= lx; ++i) AT(H, i, 0) = o + i * e;
  }
  if (mode == 3)
    for (int j = 1; j <= ly; ++j) AT(H, 0, j) = -(o + j * e);
  for (int i = 1; i <= lx; ++i)
    for (int j = 1; j <= ly; ++j) {
      AT(E, i, j) = orc_better(mn, AT(E, i - 1, j) + ee, AT(H, i - 1, j) + oe);
      AT(F, i, j) = orc_better(mn, AT(F, i, j - 1) + ee, AT(H, i, j - 1) + oe);
      int64_t h = orc_better(mn, AT(H, i - 1, j - 1) + T[(int64_t)x[i - 1] * A + y[j - 1]], orc_better(mn, AT(E, i, j), AT(F, i, j)));
      if (mode == 1 && h < 0) h = 0;
      AT(H, i, j) = h;
    }
  /* the end cell: the first of the largest among the mode's candidates, in the order by i, then j */
  int bi = lx, bj = ly;
  if (mode != 0) {
    int first = 1;
    for (int i = 0; i <= lx; ++i)
      for (int j = 0; j <= ly; ++j) {
        const int cand = mode == 1 || (mode == 2 && (i == lx || j == ly)) || (mode == 3 && j == ly);
        if (cand && (first || AT(H, i, j) > AT(H, bi, bj))) {
          bi = i;
          bj = j;
          first = 0;
        }
      }
  }
  /* the walk, codes written backwards */
  int i = bi, j = bj, state = 0, n = 0, ident = 0;
  for (;;) {
    if (state == 0) {
      if (mode == 1 && AT(H, i, j) == 0) break;
      if (mode == 2 && (i == 0 || j == 0)) break;
      if (mode == 0 && (i == 0 || j == 0)) {
        for (; j > 0 && i == 0; --j) ops[n++] = 3;
        for (; i > 0; --i) ops[n++] = 2;
        break;
      }
      if (mode == 3 && j == 0) break;
      if (mode == 3 && i == 0) {
        for (; j > 0; --j) ops[n++] = 3;
        break;
      }
      if (AT(H, i, j) == AT(H, i - 1, j - 1) + T[(int64_t)x[i - 1] * A + y[j - 1]]) {
        ops[n++] = 1;
        ident += x[i - 1] == y[j - 1];
        --i;
        --j;
      } else if (AT(H, i, j) == AT(E, i, j)) {
        state = 1;
      } else {
        state = 2;
      }
    } else if (state == 1) {
      ops[n++] = 2;
      if (AT(E, i, j) == AT(H, i - 1, j) + oe) state = 0;
      --i;
    } else {
      ops[n++] = 3;
      if (AT(F, i, j) == AT(H, i, j - 1) + oe) state = 0;
      --j;
    }
  }
  for (int a = 0, b = n - 1; a < b; ++a, --b) {
    const uint8_t t = ops[a];
    ops[a] = ops[b];
    ops[b] = t;
  }
  for (int64_t k = n; k < ldo; ++k) ops[k] = 0;
  head[0] = (int32_t)AT(H, bi, bj);
  head[1] = i;
  head[2] = bi;
  head[3] = j;
  head[4] = bj;
  head[5] = n;
  head[6] = ident;
  head[7] = 0;
#undef AT
}

int orc_align_trace(const uint8_t *X, int64_t n, int xw, const uint8_t *Y, int64_t m, int yw, const int32_t *xi, const int32_t *yi,
                    int64_t npairs, const int64_t *T, int A, int gap, int gap_open, int mode, int32_t *head, uint8_t *ops, int64_t ldo) {
  if (!X || !Y || !xi || !yi || !T || !head || !ops || xw < 1 || yw < 1 || npairs < 0 || A < 1 || A > 256 || mode < 0 || mode > 3 ||
      gap < 0 || gap_open < 0)
    return 5;
  int *xlen = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1)), *ylen = (int *)malloc(sizeof(int) * (size_t)(m > 0 ? m : 1));
  if (!xlen || !ylen) { free(xlen); free(ylen); return 6; }
  int rc = 0;
  for (int64_t r = 0; r < n; ++r) {
    xlen[r] = row_len(X + r * xw, xw);
    for (int k = 0; k < xlen[r]; ++k)
      if (X[r * xw + k] >= A) rc = 2;
  }
  for (int64_t r = 0; r < m; ++r) {
    ylen[r] = row_len(Y + r * yw, yw);
    for (int k = 0; k < ylen[r]; ++k)
      if (Y[r * yw + k] >= A) rc = 2;
  }
  int64_t most = 1;
  for (int64_t p = 0; p < npairs && !rc; ++p) {
    if (xi[p] < 0 || xi[p] >= n || yi[p] < 0 || yi[p] >= m) { rc = 1; break; }
    const int64_t cells = (int64_t)(xlen[xi[p]] + 1) * (ylen[yi[p]] + 1);
    if (cells > ORC_TRACE_MAX_CELLS) rc = 3;
    if (xlen[xi[p]] + ylen[yi[p]] > ldo) rc = 4;
    if (cells > most) most = cells;
  }
  if (!rc) {
#pragma omp parallel
    {
      int64_t *tab = (int64_t *)malloc(sizeof(int64_t) * 3 * (size_t)most);       /* this thread's H, E, F */
      if (!tab) {
#pragma omp atomic write
        rc = 6;
      }
#pragma omp for schedule(dynamic, 4)
      for (int64_t p = 0; p < npairs; ++p)
        if (tab)
          orc_trace_pair(mode, T, A, gap, gap_open, X + (int64_t)xi[p] * xw, xlen[xi[p]], Y + (int64_t)yi[p] * yw, ylen[yi[p]], tab,
                         tab + most, tab + 2 * most, head + p * 8, ops + p * ldo, ldo);
      free(tab);
    }
  }
  free(xlen);
  free(ylen);
  return rc;
}
