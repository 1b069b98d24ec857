// CPU check of the kNN launch planner (prograph_amd/csrc/pg_plan.h): no device, no runtime, no link against the library.
//   plan_check plan_table.txt
// 1. the planners against plan_table.txt: inputs and outputs of plan_mm, plan_rows, knn_plan_cost, sym_plan_host, sym_ws
//    and the workspace offsets as the code computed them before planning became a header of its own (256 CUs);
// 2. the decisions the planner's comments promise, at cfg3 and the other shapes they name;
// 3. the facts the executor relies on, over a sweep of shapes;
// 4. every knob: set alone, it changes the decisions it documents and no other.
// Last line: "plan_check ok: ..." or "plan_check FAILED: n".
#include "../../prograph_amd/csrc/pg_plan.h"

#include <stdio.h>
#include <string>
#include <vector>

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (++g_fail <= 40) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                     \
  } while (0)

// MI355X (gfx950), 256 CUs.  Resident workgroups per CU as hipOccupancyMaxActiveBlocksPerMultiprocessor reports them for the
// instances of a kNN launch, read on the device on 2026-10-21 at commit d916c5d (the library clamps the MFMA instances'
// to 4).  Order: VALU kNN, MFMA 32-row short list, MFMA 64-row short list, symmetric sweep (1: no such instance).  The MFMA
// instance with 64-lane lists (k > 19, rounds, PG_MM_SHORT=0) reports what the 32-row short-list one does, in every row
static const int kCus = 256;
static const KnnHw kOccL32B5 = {kCus, 4, 4, 4, 4};
static const KnnHw kOccL32B8 = {kCus, 4, 4, 4, 1};
static const KnnHw kOccL64B5 = {kCus, 4, 4, 4, 4};
static const KnnHw kOccL64B8 = {kCus, 3, 3, 2, 1};
static const KnnHw kOccL128B5 = {kCus, 3, 3, 3, 1};
static const KnnHw kOccL128B8 = {kCus, 2, 2, 2, 1};
static KnnHw hw_for(int l, int bits) {
  if (l <= 32) return bits == 5 ? kOccL32B5 : kOccL32B8;
  if (l <= 64) return bits == 5 ? kOccL64B5 : kOccL64B8;
  return bits == 5 ? kOccL128B5 : kOccL128B8;
}

static PgKnobs knobs(const std::vector<std::string> &env) {
  std::vector<const char *> block;
  for (const std::string &e : env) block.push_back(e.c_str());
  block.push_back(nullptr);
  return pg_knobs_read(block.data());
}
static KnnShape self_graph(int64_t n, int l = 64, int bits = 5, int k = 16) {
  KnnShape s = {};
  s.nrows = n; s.ncols = n; s.row0 = 0; s.samePlanes = true;
  s.l = l; s.bits = bits; s.k = k; s.first = 1; s.workspace = true;
  return s;
}
static KnnShape block_graph(int64_t nrows, int64_t ncols, int64_t row0 = 0) {
  KnnShape s = self_graph(nrows);
  s.ncols = ncols; s.row0 = row0;
  return s;
}

// ---------------------------------------------------------------------------------------
// 1. the table
// ---------------------------------------------------------------------------------------
static int check_table(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) { printf("cannot open %s\n", path); ++g_fail; return 0; }
  const PgKnobs kn = knobs({});
  char line[512];
  int n = 0;
  while (fgets(line, sizeof(line), f)) {
    long long a, b, c, d, e, o[8];
    double x, y;
    ++n;
    if (sscanf(line, "mm %lld %lld %lld %lld %lld = %lld %lld %lld %lld %lld %lld %lld", &a, &b, &c, &d, &e, o, o + 1, o + 2, o + 3, o + 4, o + 5, o + 6) == 12) {
      const PassPlan p = plan_mm(a, kCus, kn, (int)b, (int)c, d != 0, (int)e);
      CHECK(p.rowsPerWave == o[0] && p.rowsPerPass == o[1] && p.tailFrom == o[2] && p.tailRows == o[3] && p.passes == o[4] && p.gridWaves == o[5] && p.grid == o[6], "%s", line);
    } else if (sscanf(line, "rows %lld %lld %lld %lf %lld = %lld %lld %lld", &a, &b, &c, &x, &d, o, o + 1, o + 2) == 8) {
      const PassPlan p = plan_rows(a, b, kCus, (int)c, x, kn, (int)d);
      CHECK(p.rowsPerWave == o[0] && p.rowsPerPass == o[1] && p.grid == o[2], "%s", line);
    } else if (sscanf(line, "cost %lld %lld %lld %lld %lld = %lf %lld", &a, &b, &c, &d, &e, &y, o) == 7) {
      long long mainRows = -1;
      const double t = knn_plan_cost(a, b, kCus, (int)c, (int)d, e != 0, &mainRows);
      CHECK(t == y && mainRows == o[0], "%s-> %.17g %lld", line, t, mainRows);
    } else if (sscanf(line, "symplan %lld %lld %lld %lld = %lld", &a, &b, &c, &d, o) == 5) {
      CHECK(sym_plan_host(a, b, (int)c, (int)d, nullptr, 0) == o[0], "%s", line);
    } else if (sscanf(line, "symws %lld = %lld %lld %lld %lld %lld %lld %lld", &a, o, o + 1, o + 2, o + 3, o + 4, o + 5, o + 6) == 8) {
      const SymWs w = sym_ws(a, kCus, kn);
      CHECK(w.plan == o[0] && w.pieceStart == o[1] && w.lowCount == o[2] && w.partial == o[3] && w.lowKeys == o[4] && w.bytes == o[5] && w.maxPasses == o[6], "%s", line);
    } else if (sscanf(line, "wsoff %lld = %lld %lld %lld", &a, o, o + 1, o + 2) == 4) {
      CHECK(ws_evict_offset(a) == o[0] && ws_sym_offset(a) == o[1] && workspace_bytes(a, kCus, kn) == o[2], "%s", line);
    } else {
      CHECK(false, "unreadable line %d: %s", n, line);
    }
  }
  fclose(f);
  CHECK(n >= 2000, "only %d lines in %s", n, path);
  return n;
}

// ---------------------------------------------------------------------------------------
// 2. the promised decisions
// ---------------------------------------------------------------------------------------
static void check_promises() {
  const PgKnobs kn = knobs({});
  {  // cfg3: 200 000 rows = 3 x 65 536 + 3 392: 64-row passes, three waves per SIMD + 53 row blocks x 16 pieces, started ahead
    const KnnPlan p = knn_plan(self_graph(200000), kOccL64B5, kn);
    CHECK(p.mm && p.probe && p.shortList && p.two && p.rb == 64 && p.mode == PG_MODE_KNN_SHORT2, "cfg3 instance");
    CHECK(p.mainRows == 196608 && p.split && p.nb == 53 && p.pieces == 16, "cfg3 split: %lld %lld %d", p.mainRows, p.nb, p.pieces);
    CHECK(p.main.passes == 3072 && p.main.rowsPerWave == 64 && p.launch.passes == 3072 + 53 * 16 && p.piecesAhead && p.launch.grid == (3072 + 53 * 16) / 4, "cfg3 passes");
    CHECK(p.evict && p.sym && p.alt32 && p.guess == 10u && p.symSlots == 4096, "cfg3 sweep, alternative, cap");
    CHECK(p.mainGateMask == 1u && p.evictGateMask == (1u | 8u) && p.symGateMask == 1u, "cfg3 gates");
  }
  // x 200 000 columns: 32-row passes up to 131 072 rows; the rows of up to 128 row blocks of 32 beyond that go into column
  // pieces; from 135 169 rows on the 64-row instance is the cheaper plan
  {
    KnnPlan p = knn_plan(block_graph(131072, 200000), kOccL64B5, kn);
    CHECK(!p.two && !p.split && p.main.passes == 4096 && p.main.rowsPerWave == 32, "131 072 rows");
    p = knn_plan(block_graph(131073, 200000), kOccL64B5, kn);
    CHECK(!p.two && p.split && p.mainRows == 131072 && p.nb == 1 && p.pieces == 16 && !p.piecesAhead, "131 073 rows");
    p = knn_plan(block_graph(135168, 200000), kOccL64B5, kn);
    CHECK(!p.two && p.split && p.mainRows == 131072 && p.nb == 128 && p.pieces == 8, "135 168 rows");
    p = knn_plan(block_graph(135169, 200000), kOccL64B5, kn);
    CHECK(p.two && p.split && p.mainRows == 131072 && p.nb == 65 && !p.sym, "135 169 rows");
  }
  {  // byte alphabets (three waves per SIMD; the 64-row instance two): whole rounds of 32-row passes + pieces
    const KnnPlan p = knn_plan(self_graph(200000, 64, 8), kOccL64B8, kn);
    CHECK(p.mm && !p.two && p.split && p.mainRows == 196608 && p.nb == 106 && p.pieces == 9 && !p.sym && !p.alt32, "8-bit planes");
  }
  {  // L = 128 (three waves per SIMD) at 100 000 rows: 32-row passes + pieces
    const KnnPlan p = knn_plan(self_graph(100000, 128, 5), kOccL128B5, kn);
    CHECK(p.mm && !p.two && p.split && p.mainRows == 98304 && p.nb == 53 && p.pieces == 16 && !p.sym, "L = 128");
  }
  {  // the engines' row thresholds and caps
    CHECK(!knn_plan(self_graph(19999), kOccL64B5, kn).mm && knn_plan(self_graph(20000), kOccL64B5, kn).mm, "MFMA engine from 20 000 rows");
    CHECK(knn_plan(self_graph(4000), kOccL64B5, kn).guess == 8u && knn_plan(self_graph(24000, 32), kOccL32B5, kn).guess == 7u, "caps");
    CHECK(!knn_plan(self_graph(65535), kOccL64B5, kn).probe && knn_plan(self_graph(65536), kOccL64B5, kn).probe, "probe from 65 536 columns");
    CHECK(!use_mm_engine(27999, kn, 64, false) && use_mm_engine(28000, kn, 64, false) && !use_mm_engine(35999, kn, 32, false) && use_mm_engine(36000, kn, 32, false), "eps thresholds");
  }
}

// ---------------------------------------------------------------------------------------
// 3. the facts the executor relies on
// ---------------------------------------------------------------------------------------
static long long check_facts() {
  const PgKnobs kn = knobs({});
  std::vector<int64_t> rows = {1, 63, 64, 65, 4000, 20000, 65536, 65537, 131072, 131073, 196608, 200000, 1000000, 1ll << 24};
  unsigned long long x = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 2000; ++i) {                           // xorshift64: half of the counts uniform, half log-uniform
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    const unsigned long long u = x >> 11;
    rows.push_back(i & 1 ? 1 + (int64_t)(u % (1ull << 24)) : 1 + (int64_t)((u % (1ull << 24)) >> (u >> 40) % 12));
  }
  long long plans = 0;
  for (int64_t n : rows)                                     // (rows outermost: sym_plan_host keeps the last counts)
    for (int rect = 0; rect < 2; ++rect)
      for (int bits : {5, 8})
        for (int l : {32, 64, 128})
          for (int k : {1, 16, 63})
            for (int first = 0; first < 2; ++first)
              for (int floorKeys = 0; floorKeys < 2; ++floorKeys) {
                KnnShape s = self_graph(n, l, bits, k);
                if (rect) { s.row0 = 64; s.ncols = 2 * n + 64 < PG_MAX_N_KNN ? 2 * n + 64 : PG_MAX_N_KNN; }
                s.first = first; s.floorKeys = floorKeys != 0; s.lastKeys = floorKeys != 0 || first == 0;
                const KnnHw hw = hw_for(l, bits);
                const KnnPlan p = knn_plan(s, hw, kn);
                const int64_t ws = workspace_bytes(n, hw.cus, kn);
                ++plans;
#define SHAPE "n=%lld rect=%d bits=%d l=%d k=%d first=%d floor=%d", (long long)n, rect, bits, l, k, first, floorKeys
                CHECK(p.valu.grid > 0 && p.valu.rowsPerWave > 0 && p.valu.rowsPerPass > 0, SHAPE);
                if (!p.mm) continue;
                CHECK(p.mainRows >= 0 && p.mainRows <= n && p.split == (p.mainRows < n), SHAPE);
                CHECK(p.main.grid > 0 && p.launch.grid > 0 && p.launch.gridWaves == 4ll * p.launch.grid && p.launch.passes >= p.main.passes, SHAPE);
                if (p.split) {
                  CHECK(p.mainRows > 0 && p.nb >= 1 && p.nb <= 128 && p.pieces >= 2 && p.pieces <= 16 && p.nb * p.pieces <= 1024, SHAPE);
                  CHECK(p.nb * p.rb >= n - p.mainRows && p.nb * p.rb * p.pieces * PG_MM_KL * 4 <= PG_WS_PARTIAL_BYTES, SHAPE);
                  CHECK(PG_WS_PARTIAL + PG_WS_PARTIAL_BYTES <= p.evictOffset && n > PG_SPLIT_MIN_ROWS, SHAPE);
                  CHECK(p.pieceMergeGrid > 0 && p.evict && p.shortList && p.main.passes * p.rb == p.mainRows, SHAPE);
                }
                if (p.evict) CHECK(p.evictGrid > 0 && p.evictOffset >= PG_WS_PARTIAL && p.evictOffset + 4 * n <= ws_sym_offset(n), SHAPE);
                if (p.alt32) CHECK(p.alt.grid > 0 && p.two && p.probe, SHAPE);
                CHECK(p.symBase == ws_sym_offset(n) && p.symBase + p.symWs.bytes == ws && ws_sym_offset(n) <= ws, SHAPE);
                if (p.sym) {
                  const SymWs &w = p.symWs;
                  CHECK(!rect && bits == 5 && plan_nchunks(l, bits) <= 3 && p.shortList && p.evict && s.row0 == 0 && s.nrows == s.ncols, SHAPE);
                  CHECK(p.symPasses >= 1 && p.symPasses <= w.maxPasses && p.symSlots >= 1 && p.symGridWaves >= 4 && p.symPlanGrid >= 2 && p.symMergeGrid >= 1, SHAPE);
                  CHECK(w.plan + 16 * p.symPasses <= w.pieceStart && w.pieceStart + 4 * (p.symNb + 1) <= w.lowCount, SHAPE);
                  CHECK(w.lowCount + 16 * p.symZero4 <= w.partial && 4 * p.symZero4 >= n, SHAPE);
                  CHECK(w.partial + p.symPasses * 64 * PG_MM_KL * 4 <= w.lowKeys && w.lowKeys + n * (int64_t)p.symCapL * 4 <= w.bytes, SHAPE);
                  CHECK(p.symBase + w.bytes <= ws && p.symNb == (n + 63) / 64 && p.symNst == (n + 127) / 128, SHAPE);
                }
#undef SHAPE
              }
  return plans;
}

// ---------------------------------------------------------------------------------------
// 4. the knobs
// ---------------------------------------------------------------------------------------
enum {
  D_ENGINE = 1 << 0,    // mm
  D_GUESS = 1 << 1,     // guess
  D_PROBE = 1 << 2,     // probe
  D_SHORT = 1 << 3,     // shortList
  D_TWO = 1 << 4,       // two (64-row passes)
  D_SPLIT = 1 << 5,     // mainRows, nb
  D_PIECES = 1 << 6,    // pieces
  D_AHEAD = 1 << 7,     // piecesAhead
  D_SYM = 1 << 8,       // sym
  D_SYMPLAN = 1 << 9,   // the sweep's slots, passes, piece rule
  D_ALT32 = 1 << 10,    // alt32
  D_EVICT = 1 << 11,    // evict
  D_VALUPASS = 1 << 12, // the VALU launch's row split
  D_MMPASS = 1 << 13,   // the MFMA launches' plain passes (the main launch's compared where instance and split stand; the alternative's where both have one)
  D_ALL_MM = 1 << 14    // expectation only: the engine changes, nothing of the MFMA half is compared
};
static bool same_pass(const PassPlan &a, const PassPlan &b) {
  return a.rowsPerWave == b.rowsPerWave && a.rowsPerPass == b.rowsPerPass && a.tailFrom == b.tailFrom && a.tailRows == b.tailRows &&
         a.passes == b.passes && a.gridWaves == b.gridWaves && a.grid == b.grid;
}
static int plan_diff(const KnnPlan &a, const KnnPlan &b) {
  int d = 0;
  if (a.mm != b.mm) d |= D_ENGINE;
  if (a.guess != b.guess) d |= D_GUESS;
  if (a.probe != b.probe) d |= D_PROBE;
  if (a.shortList != b.shortList) d |= D_SHORT;
  if (a.two != b.two) d |= D_TWO;
  if (a.mainRows != b.mainRows || a.nb != b.nb || a.split != b.split) d |= D_SPLIT;
  if (a.pieces != b.pieces) d |= D_PIECES;
  if (a.piecesAhead != b.piecesAhead) d |= D_AHEAD;
  if (a.sym != b.sym) d |= D_SYM;
  if (a.symSlots != b.symSlots || a.symPasses != b.symPasses || a.symPiece != b.symPiece || a.symPieceMin != b.symPieceMin) d |= D_SYMPLAN;
  if (a.alt32 != b.alt32) d |= D_ALT32;
  if (a.evict != b.evict) d |= D_EVICT;
  if (!same_pass(a.valu, b.valu)) d |= D_VALUPASS;
  if (!(d & (D_TWO | D_SPLIT)) && !same_pass(a.main, b.main)) d |= D_MMPASS;   // (`launch` is `main` + the pieces, ahead or not)
  if (a.alt32 && b.alt32 && !same_pass(a.alt, b.alt)) d |= D_MMPASS;
  return d;
}
struct KnobCase {
  const char *env;
  int cfg3, n70k, n66k;      // the decisions that change at cfg3 (200 000 rows), at 70 000 rows and at 66 000 rows (self graphs, L = 64, 5-bit, k = 16)
};
// The defaults.  cfg3: above.  70 000 rows: MFMA engine, probe, short lists, 32-row passes (three waves per SIMD, no split:
// 4 464 rows beyond two full waves are more than 128 row blocks), no sweep.  66 000 rows: the same with 65 536 rows in plain
// passes and 15 row blocks in 16 pieces, started ahead - the shape where PG_MM_PIECES_AHEAD and the 32-row split show.
static const KnobCase kKnobCases[] = {
    {"PG_ENGINE=valu", D_ALL_MM, D_ALL_MM, D_ALL_MM},
    {"PG_ENGINE_MIN_ROWS=1000000", D_ALL_MM, D_ALL_MM, D_ALL_MM},
    // present: no probe, so no gated alternative either
    {"PG_KNN_GUESS=6", D_GUESS | D_PROBE | D_ALT32, D_GUESS | D_PROBE, D_GUESS | D_PROBE},
    {"PG_PROBE=0", D_PROBE | D_ALT32, D_PROBE, D_PROBE},
    // no short lists: no 64-row instance, no pieces, no sweep
    {"PG_MM_SHORT=0", D_SHORT | D_TWO | D_SPLIT | D_PIECES | D_AHEAD | D_SYM | D_SYMPLAN | D_ALT32, D_SHORT, D_SHORT | D_SPLIT | D_PIECES | D_AHEAD},
    // cfg3 on 32-row passes: 68 928 rows beyond one round are no pieces; the sweep and the alternative go with the 64-row instance
    {"PG_MM_R=1", D_TWO | D_SPLIT | D_PIECES | D_AHEAD | D_SYM | D_SYMPLAN | D_ALT32, 0, 0},
    // forced 64-row passes: no alternative (cfg3); two waves per SIMD hold the rows, a self graph is swept symmetrically
    {"PG_MM_R=2", D_ALT32, D_TWO | D_SYM | D_SYMPLAN, D_TWO | D_SPLIT | D_PIECES | D_AHEAD | D_SYM | D_SYMPLAN},
    {"PG_MM_SPLIT=0", D_SPLIT | D_PIECES | D_AHEAD, 0, D_SPLIT | D_PIECES | D_AHEAD},
    // no eviction: the pieces and the sweep need it
    {"PG_MM_EVICT=0", D_EVICT | D_SPLIT | D_PIECES | D_AHEAD | D_SYM | D_SYMPLAN, D_EVICT, D_EVICT | D_SPLIT | D_PIECES | D_AHEAD},
    {"PG_MM_PIECES=8", D_PIECES, 0, D_PIECES},
    {"PG_MM_PIECES_AHEAD=0", D_AHEAD, 0, D_AHEAD},
    {"PG_KNN_SYM=0", D_SYM | D_SYMPLAN, 0, 0},
    {"PG_KNN_SYM=1", 0, D_SYM | D_SYMPLAN, D_SYM | D_SYMPLAN},
    {"PG_KNN_SYM_PIECE=8", D_SYMPLAN, 0, 0},
    {"PG_KNN_SYM_PIECE_MIN=8", D_SYMPLAN, 0, 0},
    {"PG_KNN_SYM_OCC=2", D_SYMPLAN, 0, 0},
    // uniform passes in both engines; present: no pieces
    {"PG_ROWS_PER_WAVE=12", D_VALUPASS | D_MMPASS | D_SPLIT | D_PIECES | D_AHEAD, D_VALUPASS | D_MMPASS, D_VALUPASS | D_SPLIT | D_PIECES | D_AHEAD},
    // round 2's rule spreads a single round over ~97 % of the slots (cfg3: 3 933 plain passes of 50 rows, which leave no free
    // slots for the pieces to start ahead)
    {"PG_MM_PLAN=2", D_MMPASS | D_AHEAD, D_MMPASS, D_MMPASS},
    // (only with round 2's rule: eps launches - checked on plan_mm below)
    {"PG_MM_TAIL=1", 0, 0, 0},
    // one wave per pass: shows where the passes outnumber the slots - cfg3's 32-row alternative, 6 250 passes
    {"PG_MM_PERSISTENT=0", D_MMPASS, 0, 0},
};
static void check_knobs() {
  const PgKnobs dflt = knobs({});
  const int64_t sizes[3] = {200000, 70000, 66000};
  KnnPlan base[3];
  for (int i = 0; i < 3; ++i) base[i] = knn_plan(self_graph(sizes[i]), kOccL64B5, dflt);
  CHECK(base[1].mm && base[1].probe && base[1].shortList && !base[1].two && !base[1].split && !base[1].sym && !base[1].alt32 && base[1].evict && base[1].main.rowsPerWave == 24, "70 000 rows, defaults");
  CHECK(base[2].mm && base[2].probe && !base[2].two && base[2].split && base[2].mainRows == 65536 && base[2].nb == 15 && base[2].pieces == 16 && base[2].piecesAhead && !base[2].sym, "66 000 rows, defaults");
  for (const KnobCase &c : kKnobCases) {
    const PgKnobs kn = knobs({c.env});
    const int expect[3] = {c.cfg3, c.n70k, c.n66k};
    for (int i = 0; i < 3; ++i) {
      const KnnPlan p = knn_plan(self_graph(sizes[i]), kOccL64B5, kn);
      const int d = plan_diff(base[i], p);
      if (expect[i] == D_ALL_MM) CHECK(d & D_ENGINE && !p.mm && p.guess == 8u && !(d & D_VALUPASS), "%s at %lld rows: 0x%x", c.env, (long long)sizes[i], d);
      else CHECK(d == expect[i], "%s at %lld rows: changed 0x%x, expected 0x%x", c.env, (long long)sizes[i], d, expect[i]);
    }
  }
  // the values, where a knob carries one
  CHECK(knn_plan(self_graph(200000), kOccL64B5, knobs({"PG_KNN_GUESS=6"})).guess == 6u, "PG_KNN_GUESS");
  CHECK(knn_plan(self_graph(200000), kOccL64B5, knobs({"PG_MM_PIECES=8"})).pieces == 8, "PG_MM_PIECES");
  CHECK(knn_plan(self_graph(200000), kOccL64B5, knobs({"PG_MM_PIECES=17"})).pieces == 16, "PG_MM_PIECES out of range");
  CHECK(knn_plan(self_graph(200000), kOccL64B5, knobs({"PG_KNN_SYM_OCC=2"})).symSlots == 2048, "PG_KNN_SYM_OCC");
  CHECK(knn_plan(self_graph(200000), kOccL64B5, knobs({"PG_KNN_SYM_OCC=5"})).symSlots == 4096, "PG_KNN_SYM_OCC out of range");
  CHECK(knn_plan(self_graph(200000), kOccL64B5, knobs({"PG_ROWS_PER_WAVE=12"})).valu.rowsPerWave == 12, "PG_ROWS_PER_WAVE");
  CHECK(knn_plan(self_graph(30000), kOccL64B5, knobs({"PG_ENGINE_MIN_ROWS=40000"})).mm == false, "PG_ENGINE_MIN_ROWS");
  CHECK(knn_plan(self_graph(4000), kOccL64B5, knobs({"PG_ENGINE=mfma"})).mm && !knn_plan(self_graph(200000), kOccL64B5, knobs({"PG_ENGINE=mfma"})).probe, "PG_ENGINE=mfma");
  CHECK(knn_plan(self_graph(200000), kOccL64B5, knobs({"PG_ENGINE=other"})).mm && !knn_plan(self_graph(200000), kOccL64B5, knobs({"PG_ENGINE=other"})).probe, "PG_ENGINE present");
  // PG_MM_TAIL: round 2's rule (eps launches) shrinks the passes of the last round
  const PassPlan t0 = plan_mm(200000, kCus, dflt), t1 = plan_mm(200000, kCus, knobs({"PG_MM_TAIL=1"}));
  CHECK(t0.tailFrom == 6250 && t0.tailRows == 32 && t1.tailFrom == 4096 && t1.tailRows == 18 && t1.passes == 4096 + 3830, "PG_MM_TAIL: %lld %d %lld", t1.tailFrom, t1.tailRows, t1.passes);
  // presence and value are kept apart; the first entry of a name counts; other names are not looked at
  const PgKnobs k = knobs({"PATH=/bin", "PG_ROWS_PER_WAVE=0", "PG_MM_R=", "PG_MM_R=2", "PG_KNN_SYM_CAPL=1000", "PG_WAVES_PER_CU=30", "PG_MM_RUN=0", "PG_MM_RX=1"});
  CHECK(k.rowsPerWave.set && k.rowsPerWave.v == 0 && k.mmR.set && k.mmR.v == 0 && k.symCapL.v == 256 && waves_per_cu(k) == 28 && k.mmRun.v == 1 && !k.mmSplit.set && k.mmSplit.v == 1, "reader");
  CHECK(dflt.symCapL.v == 256 && dflt.symPieceMin.v == 32 && dflt.knnSym.v == -1 && dflt.gateForce.v == -1 && dflt.lbFilter.v == 1 && !dflt.debugPlan.set, "defaults");
}

int main(int argc, char **argv) {
  if (argc < 2) { printf("usage: plan_check plan_table.txt\n"); return 2; }
  const int lines = check_table(argv[1]);
  check_promises();
  const long long plans = check_facts();
  check_knobs();
  if (g_fail) { printf("plan_check FAILED: %d\n", g_fail); return 1; }
  printf("plan_check ok: %d table lines, %lld plans swept, %d knob cases\n", lines, plans, (int)(sizeof(kKnobCases) / sizeof(kKnobCases[0])));
  return 0;
}
