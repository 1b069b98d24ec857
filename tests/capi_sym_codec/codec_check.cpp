// CPU check of the entries the symmetric kNN sweep delivers (prograph_amd/csrc/pg_plan.h: sym_dist_bits, sym_row_bits,
// sym_rows_fit, sym_entry, sym_entry_place, sym_entry_key, sym_group_cap) - the text the sweep and the merge run on the
// device - and of knn_plan's decline rule.  No device, no runtime, no link against the library.
// Last line: "codec_check ok: ..." or "codec_check FAILED: n".
#include "../../prograph_amd/csrc/pg_plan.h"

#include <stdio.h>
#include <string>
#include <vector>

static int g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++g_checks;                                           \
    if (!(cond)) {                                        \
      if (++g_fail <= 40) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                     \
  } while (0)

static PgKnobs knobs(const std::vector<std::string> &env) {
  std::vector<const char *> block;
  for (const std::string &e : env) block.push_back(e.c_str());
  block.push_back(nullptr);
  return pg_knobs_read(block.data());
}

int main() {
  // the width rule: the distance field holds cap - 1, the row field is the rest of 28 bits, 24 at most (a key's index bits)
  const struct { uint32_t cap; int dBits, rowBits; } widths[] = {{1, 0, 24},  {2, 1, 24},  {3, 2, 24},  {7, 3, 24}, {10, 4, 24},
                                                                   {16, 4, 24}, {17, 5, 23}, {64, 6, 22}, {65, 7, 21}};
  for (const auto &w : widths) {
    CHECK(sym_dist_bits(w.cap) == w.dBits, "cap %u: %d distance bits", w.cap, sym_dist_bits(w.cap));
    CHECK(sym_row_bits(w.cap) == w.rowBits, "cap %u: %d row bits", w.cap, sym_row_bits(w.cap));
    CHECK(w.cap - 1u < (1u << w.dBits) && (w.cap == 1 || w.cap - 1u >= (1u << (w.dBits - 1))), "cap %u: the field is exact", w.cap);
    CHECK(4 + w.dBits + w.rowBits <= 32, "cap %u: the fields fit a word", w.cap);
    // round trip at every field edge
    const int rb = sym_row_bits(w.cap);
    const uint32_t rowMax = (1u << rb) - 1u;
    const uint32_t places[] = {0u, 15u}, ds[] = {0u, w.cap - 1u}, rows[] = {0u, 1u, rowMax - 1u, rowMax};
    for (uint32_t place : places)
      for (uint32_t d : ds)
        for (uint32_t row : rows) {
          const uint32_t e = sym_entry(place, d, row, rb);
          CHECK(sym_entry_place(e) == place, "cap %u place %u d %u row %u: place %u", w.cap, place, d, row, sym_entry_place(e));
          CHECK(sym_entry_key(e, rb) == (d << 24 | row), "cap %u place %u d %u row %u: key %08x", w.cap, place, d, row, sym_entry_key(e, rb));
        }
    // decoded keys are ordered as distance << 24 | row: by distance first, then by row, whatever the place
    const uint32_t dHi = w.cap - 1u;
    if (dHi > 0) {
      CHECK(sym_entry_key(sym_entry(15, dHi - 1, rowMax, rb), rb) < sym_entry_key(sym_entry(0, dHi, 0, rb), rb), "cap %u: distance before row", w.cap);
    }
    CHECK(sym_entry_key(sym_entry(15, dHi, rowMax - 1u, rb), rb) < sym_entry_key(sym_entry(0, dHi, rowMax, rb), rb), "cap %u: rows ascend", w.cap);
    // the decline rule: rows 0 .. n - 1 fit the field up to n = 2^rowBits
    const int64_t lim = (int64_t)1 << rb;
    CHECK(sym_rows_fit(lim - 1, w.cap) && sym_rows_fit(lim, w.cap) && !sym_rows_fit(lim + 1, w.cap), "cap %u: limit %lld", w.cap, (long long)lim);
  }
  // the default caps cover every N the kNN keys allow
  CHECK(sym_rows_fit((int64_t)1 << 24, 10) && sym_rows_fit((int64_t)1 << 24, 7), "default caps at 2^24 rows");

  // a group's log: its rows' former slots; the last group of a graph ends with the region
  CHECK(sym_group_cap(1000, 0, 256) == 4096 && sym_group_cap(1000, 976, 256) == 4096 && sym_group_cap(1000, 992, 256) == 8 * 256, "group caps of 1000 rows");
  CHECK(sym_group_cap(129, 128, 8) == 8 && sym_group_cap(129, 112, 8) == 128 && sym_group_cap(16, 16, 8) == 0, "group caps at the seams");
  for (uint32_t n : {1u, 15u, 16u, 17u, 129u, 1001u}) {
    uint64_t sum = 0;
    for (uint32_t f = 0; f < n; f += 16) {
      CHECK((uint64_t)f * 8 + sym_group_cap(n, f, 8) <= (uint64_t)n * 8, "n %u group %u stays inside the region", n, f);
      sum += sym_group_cap(n, f, 8);
    }
    CHECK(sum == (uint64_t)n * 8, "n %u: the logs tile the region", n);
  }

  // knn_plan: the forced sweep with a cap of 65 (7 distance bits, rows below 2^21) one row below, at and above the limit;
  // the rectangular path stands where it declines
  const KnnHw hw = {256, 4, 4, 4, 4};
  for (int64_t dn = -1; dn <= 1; ++dn) {
    KnnShape s = {};
    s.nrows = s.ncols = ((int64_t)1 << 21) + dn; s.row0 = 0; s.samePlanes = true;
    s.l = 64; s.bits = 5; s.k = 16; s.first = 1; s.workspace = true;
    const KnnPlan wide = knn_plan(s, hw, knobs({"PG_KNN_SYM=1", "PG_KNN_GUESS=65"}));
    CHECK(wide.mm && wide.sym == (dn <= 0), "cap 65 at 2^21 %+lld rows: sym %d", (long long)dn, (int)wide.sym);
    if (wide.sym) CHECK(wide.symRowBits == 21, "row bits %d", wide.symRowBits);
    const KnnPlan dflt = knn_plan(s, hw, knobs({"PG_KNN_SYM=1"}));
    CHECK(dflt.sym && dflt.symRowBits == 24, "default cap at 2^21 %+lld rows: sym %d", (long long)dn, (int)dflt.sym);
  }
  if (g_fail) { printf("codec_check FAILED: %d\n", g_fail); return 1; }
  printf("codec_check ok: %d checks\n", g_checks);
  return 0;
}
