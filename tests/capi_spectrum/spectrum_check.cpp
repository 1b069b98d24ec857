// Test infrastructure: prograph_amd/csrc/pg_spectrum.h - the lines the spectrum kernel runs per window - compiled for the
// host under the address and undefined-behaviour sanitizers and held against a naive k-mer counter written here with
// 64-bit arithmetic throughout.  Rows are heap blocks of exactly their length, so a window read past a row's end is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "pg_spectrum.h"

static int failures = 0;

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                      \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static int log2_of(int dims) {
  int e = 0;
  while ((1 << e) < dims) ++e;
  return e;
}

// the definition, independently: 64-bit codes, the hash as ((code + 1) * 2654435761) mod 2^32 in 64-bit arithmetic
static std::vector<int> naive(const unsigned char *t, int l, int k, int symbols, int dims) {
  uint64_t D = 1;
  for (int j = 0; j < k; ++j) D *= (uint64_t)symbols;
  if (dims) D = (uint64_t)dims;
  std::vector<int> counts((size_t)D, 0);
  for (int i = 0; i + k <= l; ++i) {
    bool ok = true;
    uint64_t code = 0;
    for (int j = 0; j < k; ++j) {
      if (t[i + j] == 0) ok = false;
      code = code * (uint64_t)symbols + (uint64_t)(t[i + j] ? t[i + j] - 1 : 0);
    }
    if (!ok) continue;
    uint64_t bucket = code;
    if (dims) bucket = (((code + 1ull) * 2654435761ull) % (1ull << 32)) >> (32 - log2_of(dims));
    CHECK(bucket < D, "naive bucket out of range");
    counts[(size_t)bucket] += 1;
  }
  return counts;
}

// the profile as the kernel forms it: pg_sp_window on every window of the row
static std::vector<int> routine(const unsigned char *t, int l, int k, int symbols, int dims) {
  const int D = pg_sp_dims(k, symbols, dims);
  std::vector<int> counts((size_t)D, 0);
  const int shift = pg_sp_shift(dims);
  for (int i = 0; i + k <= l; ++i) {
    uint32_t bucket = 0xFFFFFFFFu;
    if (pg_sp_window(t + i, k, symbols, shift, &bucket)) {
      CHECK(bucket < (uint32_t)D, "bucket %u outside 0..%d", bucket, D - 1);
      if (bucket < (uint32_t)D) counts[bucket] += 1;
    }
  }
  return counts;
}

static void compare(const unsigned char *src, int l, int k, int symbols, int dims) {
  unsigned char *row = (unsigned char *)malloc(l ? (size_t)l : 1);     // exactly l bytes under the sanitizer
  if (l) memcpy(row, src, (size_t)l);
  const std::vector<int> a = naive(row, l, k, symbols, dims), b = routine(row, l, k, symbols, dims);
  CHECK(a.size() == b.size(), "width %zu vs %zu (k %d, symbols %d, dims %d)", b.size(), a.size(), k, symbols, dims);
  if (a.size() == b.size())
    for (size_t d = 0; d < a.size(); ++d)
      if (a[d] != b[d]) {
        CHECK(false, "l %d k %d symbols %d dims %d: bucket %zu holds %d, expected %d", l, k, symbols, dims, d, b[d], a[d]);
        break;
      }
  free(row);
}

int main() {
  // ---- the widths
  CHECK(pg_sp_dims(3, 20, 0) == 8000 && pg_sp_dims(3, 32, 0) == 32768 && pg_sp_dims(3, 33, 0) == -1, "exact widths");
  CHECK(pg_sp_dims(6, 20, 1024) == 1024 && pg_sp_dims(6, 31, 32768) == 32768 && pg_sp_dims(1, 2, 0) == 2, "hashed widths");
  CHECK(pg_sp_dims(0, 20, 0) == -1 && pg_sp_dims(7, 2, 0) == -1 && pg_sp_dims(2, 1, 0) == -1 && pg_sp_dims(2, 256, 0) == -1, "k, symbols");
  CHECK(pg_sp_dims(6, 36, 64) == -1 && pg_sp_dims(4, 215, 64) == 64 && pg_sp_dims(4, 216, 64) == -1, "symbols^k <= 2^31");
  CHECK(pg_sp_dims(2, 20, 32) == -1 && pg_sp_dims(2, 20, 65536) == -1 && pg_sp_dims(2, 20, 96) == -1 && pg_sp_dims(2, 20, -64) == -1, "dims");
  for (int dims = 64; dims <= 32768; dims *= 2) CHECK(pg_sp_shift(dims) == 32 - log2_of(dims), "shift of %d", dims);
  CHECK(pg_sp_shift(0) == 0, "shift of the exact mode");

  // ---- every sequence over {0, 1, 2} and {0, 1, 2, 3} of lengths 0..7, k = 1..4, exact and dims = 64
  long long cases = 0;
  for (int symbols = 2; symbols <= 3; ++symbols)
    for (int l = 0; l <= 7; ++l) {
      long long total = 1;
      for (int j = 0; j < l; ++j) total *= symbols + 1;
      for (long long s = 0; s < total; ++s) {
        unsigned char t[8] = {0};
        long long v = s;
        for (int j = 0; j < l; ++j) { t[j] = (unsigned char)(v % (symbols + 1)); v /= symbols + 1; }
        for (int k = 1; k <= 4; ++k) {
          compare(t, l, k, symbols, 0);
          compare(t, l, k, symbols, 64);
          cases += 2;
        }
      }
    }

  // ---- random rows: lengths {0, k-1, k, k+1, 63, 64, 65, 2048}, symbols {2, 20, 31, 255}, k up to 6 wherever
  // symbols^k <= 2^31; exact wherever it is at most 32768, hashed at the two ends and the middle of the dims range.
  // One row in three is clean, one has scattered zeros, one is a single repeated letter (the largest count).
  const int syms[4] = {2, 20, 31, 255}, hashed[3] = {64, 1024, 32768};
  std::vector<unsigned char> buf(2048);
  for (int si = 0; si < 4; ++si)
    for (int k = 1; k <= 6; ++k) {
      const int symbols = syms[si];
      if (pg_sp_dims(k, symbols, 64) < 0) continue;
      const int lens[8] = {0, k - 1, k, k + 1, 63, 64, 65, 2048};
      for (int li = 0; li < 8; ++li)
        for (int kind = 0; kind < 3; ++kind) {
          const int l = lens[li];
          const unsigned char one = (unsigned char)(1 + rnd() % symbols);
          for (int i = 0; i < l; ++i) {
            unsigned char t = kind == 2 ? one : (unsigned char)(1 + rnd() % symbols);
            if (kind == 1 && rnd() % 7 == 0) t = 0;
            buf[i] = t;
          }
          if (l && kind == 0) buf[l - 1] = (unsigned char)symbols;          // the last letter: the highest codes
          if (pg_sp_dims(k, symbols, 0) > 0) { compare(buf.data(), l, k, symbols, 0); ++cases; }
          for (int h = 0; h < 3; ++h) { compare(buf.data(), l, k, symbols, hashed[h]); ++cases; }
        }
    }

  // ---- the hash alone against the formula in 64-bit arithmetic, at the ends of the code range
  for (int dims = 64; dims <= 32768; dims *= 2) {
    const unsigned char lo[6] = {1, 1, 1, 1, 1, 1}, hi[6] = {31, 31, 31, 31, 31, 31};
    uint32_t b = 0;
    CHECK(pg_sp_window(lo, 6, 31, pg_sp_shift(dims), &b) && b == (uint32_t)((2654435761ull % (1ull << 32)) >> (32 - log2_of(dims))), "hash of code 0");
    const uint64_t top = 887503681ull;                                      // 31^6: the code of hi is top - 1
    CHECK(pg_sp_window(hi, 6, 31, pg_sp_shift(dims), &b) && b == (uint32_t)(((top * 2654435761ull) % (1ull << 32)) >> (32 - log2_of(dims))),
          "hash of the highest code");
  }
  // a token above `symbols` never yields a bucket
  {
    const unsigned char t[3] = {1, 21, 2};
    uint32_t b = 0;
    CHECK(!pg_sp_window(t, 3, 20, 0, &b) && !pg_sp_window(t + 1, 2, 20, pg_sp_shift(64), &b) && pg_sp_window(t + 2, 1, 20, 0, &b) && b == 1u,
          "a token above symbols is skipped");
  }

  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("spectrum routines OK (%lld profiles compared)\n", cases);
  return 0;
}
