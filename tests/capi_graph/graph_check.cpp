// The host-and-device routines of prograph_amd/csrc/pg_graph.h on the host, under -fsanitize=address,undefined:
//   - the sorting network: every step's pairs are disjoint and cover the block (so 256 lanes may take them in any order); the wave
//     form (tier 1) at every length 0..64; the workgroup form (tiers 2 and 3) at every length 0..130 with chunks of 4, 8, 64 and
//     4096 keys, at limit-1, limit, limit+1 of each tier and at 70 000 keys - in arrays of exactly the segment's length and the
//     chunk's size, so that a pair past the length or outside the chunk is an error of the address sanitizer;
//   - the merge ranks and the run combine on every pair of ascending lists over columns 0..3 of lengths 0..4, duplicates among
//     them, both modes, both combines, every weight kind, NaN and +-0 among the floats, against a brute-force reading of the
//     definition; the winner of two weights is checked to be symmetric and the fold to be independent of its order;
//   - binary16 -> float on all 65 536 patterns; the row search over empty rows.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pg_graph.h"

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                     \
  } while (0)

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

struct NoSync { void operator()() const {} };

// distinct keys in a random order; `near_inf`: the largest key forms among them
static std::vector<pg_u64> distinct_keys(long long n, bool near_inf) {
  std::vector<pg_u64> k((size_t)n);
  for (long long i = 0; i < n; ++i) k[(size_t)i] = near_inf ? (PG_NO_COLUMN << 32 | (pg_u64)i) - (i & 1 ? 0 : (1ull << 40)) : (pg_u64)i * 3 + 1;
  for (long long i = n - 1; i > 0; --i) std::swap(k[(size_t)i], k[(size_t)(rnd() % (unsigned long long)(i + 1))]);
  return k;
}

static void check_schedule() {
  for (long long P = 2; P <= 256; P <<= 1)
    for (long long k = 2; k <= P; k <<= 1)
      for (long long j = k / 2; j > 0; j >>= 1) {
        std::vector<int> seen((size_t)P, 0);
        for (long long t = 0; t < P / 2; ++t) {
          long long lo, hi;
          pg_bitonic_pair(t, k, j, &lo, &hi);
          CHECK(lo >= 0 && lo < hi && hi < P, "pair %lld of (%lld, %lld): %lld %lld", t, k, j, lo, hi);
          CHECK(pg_bitonic_partner(lo, k, j) == hi && pg_bitonic_partner(hi, k, j) == lo, "partner is no involution");
          CHECK(lo / k == hi / k, "a pair leaves its block of k");
          if (lo >= 0 && hi < P) { seen[(size_t)lo]++; seen[(size_t)hi]++; }
        }
        for (long long i = 0; i < P; ++i) CHECK(seen[(size_t)i] == 1, "index %lld in %d pairs of (%lld, %lld)", i, seen[(size_t)i], k, j);
      }
  CHECK(pg_pow2_ceil(0) == 1 && pg_pow2_ceil(1) == 1 && pg_pow2_ceil(2) == 2 && pg_pow2_ceil(3) == 4 && pg_pow2_ceil(4096) == 4096 &&
        pg_pow2_ceil(4097) == 8192, "pow2_ceil");
}

static void check_wave_form() {
  for (int n = 0; n <= PG_GRAPH_T1; ++n)
    for (int pass = 0; pass < 2; ++pass) {
      std::vector<pg_u64> keys = distinct_keys(n, pass == 1), want = keys;
      std::sort(want.begin(), want.end());
      pg_u64 lane[64], next[64];
      for (int l = 0; l < 64; ++l) lane[l] = l < n ? keys[(size_t)l] : PG_KEY_INF;
      const int P = (int)pg_pow2_ceil(n);
      for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int l = 0; l < 64; ++l) {
            const int partner = (int)pg_bitonic_partner(l, k, j);
            CHECK(partner >= 0 && partner < 64, "a lane outside the wave");
            next[l] = pg_wave_keep(lane[l], lane[partner & 63], l, partner);
          }
          memcpy(lane, next, sizeof(lane));
        }
      for (int l = 0; l < n; ++l) CHECK(lane[l] == want[(size_t)l], "wave form, n = %d, lane %d", n, l);
      for (int l = n; l < 64; ++l) CHECK(lane[l] == PG_KEY_INF, "wave form, n = %d: the padding moved", n);
    }
}

static void check_block_form_at(long long n, long long T2) {
  std::vector<pg_u64> keys = distinct_keys(n, (n & 3) == 3), want = keys;
  std::sort(want.begin(), want.end());
  const long long P = pg_pow2_ceil(n), C = P < T2 ? P : T2;
  pg_u64 *g = (pg_u64 *)malloc((size_t)(n ? n : 1) * sizeof(pg_u64));       // exactly n: a pair past the length is caught
  pg_u64 *chunk = (pg_u64 *)malloc((size_t)C * sizeof(pg_u64));
  if (n) memcpy(g, keys.data(), (size_t)n * sizeof(pg_u64));
  pg_block_sort(g, chunk, n, T2, 0, 1, NoSync());
  CHECK(n == 0 || memcmp(g, want.data(), (size_t)n * sizeof(pg_u64)) == 0, "block form, n = %lld, T2 = %lld", n, T2);
  free(g);
  free(chunk);
}

static void check_block_form() {
  const long long chunks[] = {4, 8, 64, PG_GRAPH_T2};
  for (long long T2 : chunks)
    for (long long n = 0; n <= 130; ++n) check_block_form_at(n, T2);
  const long long seams[] = {PG_GRAPH_T1 - 1, PG_GRAPH_T1, PG_GRAPH_T1 + 1, PG_GRAPH_T2 - 1, PG_GRAPH_T2, PG_GRAPH_T2 + 1,
                             2 * PG_GRAPH_T2 - 1, 2 * PG_GRAPH_T2, 2 * PG_GRAPH_T2 + 1, 3 * PG_GRAPH_T2 + 5, 70000};
  for (long long n : seams) check_block_form_at(n, PG_GRAPH_T2);
  for (long long n : {255ll, 256ll, 257ll, 1000ll, 1025ll}) check_block_form_at(n, 64);
}

// ------------------------------------------------------------------------------------------------ weights
static float half_reference(unsigned h) {
  const int sign = (h >> 15) & 1, ex = (h >> 10) & 31, man = h & 0x3FF;
  double v;
  if (ex == 31) v = man ? NAN : INFINITY;
  else if (ex == 0) v = std::ldexp((double)man, -24);
  else v = std::ldexp((double)(man + 1024), ex - 25);
  return (float)(sign ? -v : v);
}

static void check_half() {
  for (unsigned h = 0; h < 65536; ++h) {
    const float got = pg_half_bits_to_float(h), want = half_reference(h);
    if (want != want) {
      unsigned bits;
      memcpy(&bits, &got, 4);
      CHECK(got != got && (bits >> 31) == (h >> 15), "half %04x: NaN expected", h);
    } else {
      CHECK(memcmp(&got, &want, 4) == 0, "half %04x: %g, not %g", h, got, want);
    }
  }
}

struct Kind { int eb, kind; };
static const Kind KINDS[] = {{1, PG_W_UNSIGNED}, {2, PG_W_SIGNED}, {4, PG_W_SIGNED}, {2, PG_W_FLOAT}, {4, PG_W_FLOAT}};

// the definition, written apart from pg_w_pick: values as doubles, NaN apart, the tie rule on the bits
static double value_of(unsigned bits, Kind kd, bool *nan) {
  *nan = false;
  if (kd.kind == PG_W_UNSIGNED) return (double)bits;
  if (kd.kind == PG_W_SIGNED) return kd.eb == 1 ? (double)(int8_t)bits : kd.eb == 2 ? (double)(int16_t)bits : (double)(int32_t)bits;
  float f;
  if (kd.eb == 2) f = half_reference(bits); else memcpy(&f, &bits, 4);
  *nan = f != f;
  return (double)f;
}
static unsigned pick_reference(unsigned a, unsigned b, Kind kd, int combine) {
  bool na, nb;
  const double x = value_of(a, kd, &na), y = value_of(b, kd, &nb);
  if (na && nb) return std::min(a, b);
  if (na) return b;
  if (nb) return a;
  if (x == y) return std::min(a, b);
  return ((x < y) == (combine == PG_COMBINE_MIN)) ? a : b;
}

static std::vector<unsigned> palette(Kind kd) {
  if (kd.kind == PG_W_UNSIGNED) return {0, 1, 7, 200, 255};
  if (kd.kind == PG_W_SIGNED && kd.eb == 2) return {0, 1, 0x7FFF, 0x8000, 0xFFFF, 0xFFF0, 300};
  if (kd.kind == PG_W_SIGNED) return {0, 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 0xFFFF0000u, 70000};
  if (kd.eb == 2) return {0x0000, 0x8000, 0x3C00, 0xBC00, 0x0001, 0x8001, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0x4248};
  return {0x00000000u, 0x80000000u, 0x3F800000u, 0xBF800000u, 0x00000001u, 0x80000001u, 0x7F800000u, 0xFF800000u,
          0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0x40490FDBu};
}

static void check_pick() {
  for (Kind kd : KINDS) {
    CHECK(pg_w_kind_ok(kd.eb, kd.kind), "a kind the containers carry is refused");
    const std::vector<unsigned> p = palette(kd);
    for (int combine = 0; combine < 2; ++combine)
      for (unsigned a : p)
        for (unsigned b : p) {
          const unsigned got = pg_w_pick(a, b, kd.eb, kd.kind, combine);
          CHECK(got == pick_reference(a, b, kd, combine), "pick(%x, %x) of (%d, %d) combine %d: %x", a, b, kd.eb, kd.kind, combine, got);
          CHECK(got == pg_w_pick(b, a, kd.eb, kd.kind, combine), "pick is not symmetric at (%x, %x)", a, b);
          for (unsigned c : p)          // associative: a fold does not depend on its order
            CHECK(pg_w_pick(pg_w_pick(a, b, kd.eb, kd.kind, combine), c, kd.eb, kd.kind, combine) ==
                      pg_w_pick(a, pg_w_pick(b, c, kd.eb, kd.kind, combine), kd.eb, kd.kind, combine),
                  "pick is not associative at (%x, %x, %x)", a, b, c);
        }
  }
  CHECK(!pg_w_kind_ok(1, PG_W_FLOAT) && !pg_w_kind_ok(3, PG_W_SIGNED) && !pg_w_kind_ok(8, PG_W_SIGNED) && !pg_w_kind_ok(4, 3) &&
        !pg_w_kind_ok(4, -1) && !pg_w_kind_ok(0, 0), "a bad kind passes");
  // +0 over -0, a number over a NaN, the smaller NaN, under min and max alike
  for (int combine = 0; combine < 2; ++combine) {
    CHECK(pg_w_pick(0x80000000u, 0u, 4, PG_W_FLOAT, combine) == 0u, "+0 wins over -0");
    CHECK(pg_w_pick(0x7FC00000u, 0xBF800000u, 4, PG_W_FLOAT, combine) == 0xBF800000u, "a number wins over a NaN");
    CHECK(pg_w_pick(0xFFC00000u, 0x7FC00000u, 4, PG_W_FLOAT, combine) == 0x7FC00000u, "the smaller NaN wins");
    CHECK(pg_w_pick(0x8000u, 0u, 2, PG_W_FLOAT, combine) == 0u && pg_w_pick(0x7E00u, 0xFC00u, 2, PG_W_FLOAT, combine) == 0xFC00u, "fp16");
  }
  CHECK(pg_w_pick(0xFFFFu, 1u, 2, PG_W_SIGNED, PG_COMBINE_MIN) == 0xFFFFu && pg_w_pick(0xFFu, 1u, 1, PG_W_UNSIGNED, PG_COMBINE_MIN) == 1u,
        "integers compare as integers of their kind");
}

// ------------------------------------------------------------------------------------------------ merge and combine
static void lists(std::vector<std::vector<int>> *out) {
  for (int len = 0; len <= 4; ++len) {
    std::vector<int> v((size_t)len, 0);
    for (;;) {
      out->push_back(v);
      int i = len - 1;
      while (i >= 0 && v[(size_t)i] == 3) --i;
      if (i < 0) break;
      const int to = v[(size_t)i] + 1;
      for (int q = i; q < len; ++q) v[(size_t)q] = to;
    }
  }
}

static void check_merge() {
  std::vector<std::vector<int>> all;
  lists(&all);
  CHECK(all.size() == 70, "%zu ascending lists over 0..3 of lengths 0..4", all.size());
  for (Kind kd : KINDS) {
    const std::vector<unsigned> pal = palette(kd);
    for (size_t ia = 0; ia < all.size(); ++ia)
      for (size_t it = 0; it < all.size(); ++it) {
        const std::vector<int> &A = all[ia], &T = all[it];
        const long long na = (long long)A.size(), nt = (long long)T.size(), len = na + nt;
        std::vector<unsigned> wa((size_t)na), wt((size_t)nt);
        for (auto &w : wa) w = pal[rnd() % pal.size()];
        for (auto &w : wt) w = pal[rnd() % pal.size()];
        // exactly len entries each: a rank past the row is the sanitizer's
        std::vector<int> col((size_t)len, -7);
        std::vector<unsigned> wb((size_t)len, 0);
        std::vector<unsigned char> side((size_t)len, 0);
        for (long long i = 0; i < na; ++i) {
          const long long p = i + pg_lower_bound(T.data(), nt, A[(size_t)i]);
          CHECK(p >= 0 && p < len && side.at((size_t)p) == 0, "rank of a_%lld", i);
          col.at((size_t)p) = A[(size_t)i]; wb.at((size_t)p) = wa[(size_t)i]; side.at((size_t)p) = PG_SIDE_A;
        }
        for (long long j = 0; j < nt; ++j) {
          const long long p = j + pg_upper_bound(A.data(), na, T[(size_t)j]);
          CHECK(p >= 0 && p < len && side.at((size_t)p) == 0, "rank of t_%lld", j);
          col.at((size_t)p) = T[(size_t)j]; wb.at((size_t)p) = wt[(size_t)j]; side.at((size_t)p) = PG_SIDE_T;
        }
        for (long long p = 1; p < len; ++p)
          CHECK(col[(size_t)p - 1] < col[(size_t)p] || (col[(size_t)p - 1] == col[(size_t)p] && side[(size_t)p - 1] <= side[(size_t)p]),
                "the merged row is not ascending with A's entries first");
        for (int mode = 0; mode < 2; ++mode)
          for (int combine = 0; combine < 2; ++combine) {
            std::vector<int> got_c, want_c;
            std::vector<unsigned> got_w, want_w;
            for (long long p = 0; p < len; ++p)
              if (p == 0 || col[(size_t)p - 1] != col[(size_t)p]) {
                int sides;
                const unsigned w = pg_run_combine(col.data(), wb.data(), side.data(), p, len, kd.eb, kd.kind, combine, &sides);
                if (pg_run_kept(sides, mode)) { got_c.push_back(col[(size_t)p]); got_w.push_back(w); }
              }
            for (int c = 0; c <= 3; ++c) {                    // the definition, column by column, folded from the far end
              std::vector<unsigned> ws;
              bool inA = false, inT = false;
              for (long long i = 0; i < na; ++i) if (A[(size_t)i] == c) { ws.push_back(wa[(size_t)i]); inA = true; }
              for (long long j = 0; j < nt; ++j) if (T[(size_t)j] == c) { ws.push_back(wt[(size_t)j]); inT = true; }
              if (mode == PG_SYM_UNION ? !(inA || inT) : !(inA && inT)) continue;
              unsigned w = ws.back();
              for (size_t q = ws.size() - 1; q-- > 0;) w = pick_reference(ws[q], w, kd, combine);
              want_c.push_back(c); want_w.push_back(w);
            }
            CHECK(got_c == want_c && got_w == want_w, "lists %zu and %zu, kind (%d, %d), mode %d, combine %d", ia, it, kd.eb, kd.kind,
                  mode, combine);
          }
      }
  }
}

static void check_row_of() {
  const long long indptr[] = {0, 0, 3, 3, 3, 4, 9, 9};      // rows 0, 2, 3, 6 are empty
  const long long want[] = {1, 1, 1, 4, 5, 5, 5, 5, 5};
  for (long long e = 0; e < 9; ++e) CHECK(pg_row_of(indptr, 7, e) == want[e], "row of entry %lld", e);
  const long long one[] = {0, 5};
  CHECK(pg_row_of(one, 1, 0) == 0 && pg_row_of(one, 1, 4) == 0, "a single row");
}

static void check_store() {
  unsigned char b[8]; unsigned short h[4]; unsigned w[2];
  memset(b, 0xEE, 8); memset(h, 0xEE, 8); memset(w, 0xEE, 8);
  pg_w_store(b, 3, 1, 0x1FFu); pg_w_store(h, 1, 2, 0x1ABCDu); pg_w_store(w, 1, 4, 0xDEADBEEFu);
  CHECK(b[3] == 0xFF && b[2] == 0xEE && b[4] == 0xEE && h[1] == 0xABCD && h[0] == 0xEEEE && h[2] == 0xEEEE && w[1] == 0xDEADBEEFu, "store");
  CHECK(pg_w_load(b, 3, 1) == 0xFFu && pg_w_load(h, 1, 2) == 0xABCDu && pg_w_load(w, 1, 4) == 0xDEADBEEFu, "load");
}

int main() {
  check_schedule();
  check_wave_form();
  check_block_form();
  check_half();
  check_pick();
  check_merge();
  check_row_of();
  check_store();
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("graph routines OK\n");
  return 0;
}
