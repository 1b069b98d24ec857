// Host-side planning of the all-pairs Hamming launches: the workspace layout, the pass planners, the plan of the symmetric
// kNN sweep, the PG_* knobs and knn_plan(), which takes every decision of a kNN launch.  Plain C++17 without a HIP header:
// everything here is a pure function of the shape, the hardware numbers (CUs, resident workgroups per CU) and the knobs, so
// tests/capi_plan checks it on the CPU.  pg_api.hip gathers those inputs and executes the plan.
#pragma once
#include "../../include/prograph_hip.h"

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>

#ifdef __HIPCC__
#define PG_HD __host__ __device__   // routines pg_knn_sym_plan_kernel runs as well
#else
#define PG_HD
#endif

// The engine's constants the planner counts with.  pg_api.hip has them from pg_common.h / pg_mm.h before it includes this
// header; a host-only build takes the copies here, and the assertion below holds both to the same values.
#ifndef PG_MODE_KNN_SHORT
enum { PG_MODE_EPS = 0, PG_MODE_KNN = 1, PG_MODE_EPS_SYM = 2 };
#define PG_MODE_KNN_SHORT 3
#define PG_MODE_KNN_SHORT2 4
#define PG_WG_WAVES 4
#define PG_RB 32
#define PG_RB_KNN 28
#define PG_MM_KL 20
#define PG_MM_RB 32
#define PG_MM_ST 128
#define PG_MM_DENSE_L1 56
#define PG_MM_DENSE_L2 48
#define PG_MM_DIRECT_RUN 8
#define PG_SYM_MAX_PIECES 16
#define PG_SYM_MAX_CAPL 256
#endif
static_assert(PG_MODE_KNN == 1 && PG_MODE_KNN_SHORT == 3 && PG_MODE_KNN_SHORT2 == 4 && PG_WG_WAVES == 4 && PG_RB == 32 &&
                  PG_RB_KNN == 28 && PG_MM_KL == 20 && PG_MM_RB == 32 && PG_MM_ST == 128 && PG_MM_DENSE_L1 == 56 &&
                  PG_MM_DENSE_L2 == 48 && PG_MM_DIRECT_RUN == 8 && PG_SYM_MAX_PIECES == 16 && PG_SYM_MAX_CAPL == 256,
              "pg_plan.h: the host-only copies of the engine's constants follow pg_common.h and pg_mm.h");

// ---------------------------------------------------------------------------------------
// Delivered keys of the symmetric kNN sweep (pg_mm.h KS, pg_knn_sym_merge_kernel).  Sixteen consecutive
// receiver rows are a GROUP: group g = row >> 4 owns the words [16 g capL, 16 g capL + sym_group_cap) of the lowKeys region
// - the sixteen rows' former slots - as one append log, and word 16 g of the lowCount region as its counter.  An entry is
// 4 bytes: the receiver's place in its group (4 bits) | the distance (dBits = bits of cap - 1: delivered distances are below
// the cap) | the sender row (the other 28 - dBits bits, 24 at most).  The widths are constants of a launch: the host plan computes the
// row field's, knn_plan declines the sweep where a row does not fit it, and sweep and merge run the text below.
// ---------------------------------------------------------------------------------------
PG_HD static inline int sym_dist_bits(uint32_t cap) {
  int b = 0;
  for (uint32_t v = cap > 0 ? cap - 1u : 0u; v; v >>= 1) ++b;
  return b;
}
// (a key has 24 index bits: caps up to 16 leave the row field at those, and the entry is the key under its place)
PG_HD static inline int sym_row_bits(uint32_t cap) { return 28 - sym_dist_bits(cap) < 24 ? 28 - sym_dist_bits(cap) : 24; }
// rows 0 .. n - 1 fit the row field
PG_HD static inline bool sym_rows_fit(int64_t n, uint32_t cap) {
  const int rb = sym_row_bits(cap);
  return rb >= 1 && n <= ((int64_t)1 << rb);
}
PG_HD static inline uint32_t sym_entry(uint32_t place, uint32_t d, uint32_t row, int rowBits) { return place << 28 | d << rowBits | row; }
PG_HD static inline uint32_t sym_entry_place(uint32_t e) { return e >> 28; }
// ... back to distance << 24 | sender row, the key order of the rectangular sweep
PG_HD static inline uint32_t sym_entry_key(uint32_t e, int rowBits) {
  return ((e & 0x0FFFFFFFu) >> rowBits) << 24 | (e & ((1u << rowBits) - 1u));
}
// entries the log of the group from row `first` (a multiple of 16) holds: its rows' capL words each (a last group of fewer
// than sixteen rows ends with the region)
PG_HD static inline uint32_t sym_group_cap(uint32_t n, uint32_t first, uint32_t capL) {
  const uint32_t rows = n > first ? n - first : 0u;
  return (rows < 16u ? rows : 16u) * capL;
}
// The merge's rounds on a lane's sixteen delivered keys, d[0] <= ... <= d[15] (no entry = 0xFFFFFFFF last).  The head of the
// list is d[0]; only a WINDOW of W keys, d[0 .. W - 1], moves when the head wins: W selects and an add a round, not sixteen.
// `used` counts the wins since the window was filled; at used == W the window holds no entry at all and the next W keys
// stand right behind it: the refill moves d[W ..] down by W (no entry at the top) - the cold path, taken by a wave where a
// ballot finds such a lane.  Between a pop and the refill that follows it d[0] is read by nobody, so d[0] is the head of the
// same sorted list in every round.  Lane-local, without a branch: the kernel and tests/capi_sym_window run this text.
#define PG_SYM_NONE 0xFFFFFFFFu
template <int W> PG_HD static inline void sym_window_pop(uint32_t (&d)[16], int &used, bool win) {
  static_assert(W == 1 || W == 2 || W == 4 || W == 16, "window widths that divide sixteen");
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int j = 0; j < W - 1; ++j) d[j] = win ? d[j + 1] : d[j];
  d[W - 1] = win ? PG_SYM_NONE : d[W - 1];
  used += win ? 1 : 0;
}
template <int W> PG_HD static inline bool sym_window_empty(int used) { return W < 16 && used == W; }
template <int W> PG_HD static inline void sym_window_refill(uint32_t (&d)[16], int &used) {
  const bool full = sym_window_empty<W>(used);
#ifdef __HIPCC__
#pragma unroll
#endif
  for (int j = 0; j < 16; ++j) d[j] = full ? (j + W < 16 ? d[j + W < 16 ? j + W : 15] : PG_SYM_NONE) : d[j];
  used = full ? 0 : used;
}

#define PG_PROBE_ROWS 64        // sample rows
#define PG_PROBE_WAVES 128      // waves per sample row: every 8th column tile (PG_PROBE_STRIDE), one turn of four tiles each at N = 200k
                                // (a turn = one L2 / Infinity-Cache round trip, ~2 us: 1 x 1 wave 206 us, 64 x 4 67 us, 64 x 32 22 us)
#define PG_PROBE_MIN_N 65536    // launches below this are not probed: the probe (~20 us) would show, and the size rules hold

static inline int plan_ngroups(int l) { return l <= 0 ? 1 : (l + 31) / 32; }
static inline int plan_nchunks(int l, int bits) { return (plan_ngroups(l) * bits + 3) / 4; }

// =======================================================================================
// The knobs: every PG_* environment variable pg_api.hip consults, in ONE table.  pg_knobs_read fills a PgKnobs from an
// environment block once per C-ABI call (not cached: tests and tools set knobs between calls of one process); nothing
// else in pg_api.hip looks at the environment.  A knob keeps apart whether the variable is PRESENT (`set`: several
// decisions test just that) and its value (`v`: the default where it is absent or, for a RANGE knob, out of range).
// =======================================================================================
struct PgKnob {
  bool set;
  long long v;
};
struct PgKnobs {
  PgKnob lbFilter, wavesPerCu, rowsPerWave, debugPlan, engine, engineMinRows, probe, probeS, probeW, gateForce, epsOrdered;
  PgKnob knnGuess, mmShort, mmR, mmSplit, mmEvict, mmPieces, mmPiecesAhead, mmPlan, mmTail, mmPersistent, mmL1, mmL2, mmRun;
  PgKnob knnSym, symCapL, symPiece, symPieceMin, symOcc, symDeliver, symEvictLimit, symMergeWgs, symMergeWindow;
};
enum { PG_ENGINE_AUTO = 0, PG_ENGINE_MFMA = 1, PG_ENGINE_VALU = 2 };
// how a value is taken: ANY as it is; CLAMP into [lo, hi]; RANGE only inside [lo, hi], the default otherwise; WIDE as ANY, read as
// a 64-bit number; NAME "mfma" / "valu" -> PG_ENGINE_MFMA / _VALU, anything else PG_ENGINE_AUTO (but present)
enum PgKnobRule { PG_KNOB_ANY, PG_KNOB_CLAMP, PG_KNOB_RANGE, PG_KNOB_WIDE, PG_KNOB_NAME };
struct PgKnobSpec {
  const char *name;
  PgKnob PgKnobs::*field;
  long long dflt, lo, hi;
  PgKnobRule rule;
  const char *what;
};
#define PG_KNOB_MAX 0x7fffffffll
static const PgKnobSpec kPgKnobs[] = {
    {"PG_LB_FILTER", &PgKnobs::lbFilter, 1, 0, 0, PG_KNOB_ANY, "stage-1 lower-bound filter: 1 adaptive, 0 off, 2 forced on"},
    {"PG_WAVES_PER_CU", &PgKnobs::wavesPerCu, 32, 4, 128, PG_KNOB_CLAMP, "VALU engine: size the row split for this many waves per CU (multiples of 4) instead of the cost rule"},
    {"PG_ROWS_PER_WAVE", &PgKnobs::rowsPerWave, 0, 1, PG_KNOB_MAX, PG_KNOB_RANGE, "uniform passes of that many rows (tuning sweeps); present: no column pieces, eps sym by plan_rows"},
    {"PG_DEBUG_PLAN", &PgKnobs::debugPlan, 0, 0, 0, PG_KNOB_ANY, "present: the [pg plan ...] lines on stderr"},
    {"PG_ENGINE", &PgKnobs::engine, PG_ENGINE_AUTO, 0, 0, PG_KNOB_NAME, "mfma / valu forces an engine; present: no probe"},
    {"PG_ENGINE_MIN_ROWS", &PgKnobs::engineMinRows, 0, 0, 0, PG_KNOB_WIDE, "rows from which the MFMA engine runs (default by kind of launch: use_mm_engine); present: no probe"},
    {"PG_PROBE", &PgKnobs::probe, 1, 0, 0, PG_KNOB_ANY, "0: no data probe, the size rules alone"},
    {"PG_PROBE_S", &PgKnobs::probeS, 0, 1, PG_PROBE_ROWS, PG_KNOB_RANGE, "sample rows of the probe (experiments)"},
    {"PG_PROBE_W", &PgKnobs::probeW, 0, 1, PG_PROBE_WAVES, PG_KNOB_RANGE, "waves per sample row of the probe (experiments)"},
    {"PG_GATE_FORCE", &PgKnobs::gateForce, -1, 0, 0, PG_KNOB_ANY, "the probe's decision is forced (tests): bit 0 gate[0], bit 1 gate[1]"},
    {"PG_EPS_ORDERED", &PgKnobs::epsOrdered, 0, 0, 0, PG_KNOB_ANY, "not 0: eps slots in column order (NsqParams::epsOrdered)"},
    {"PG_KNN_GUESS", &PgKnobs::knnGuess, 0, 0, 0, PG_KNOB_ANY, "the optimistic stage-1 cap (default by engine and length); present: no probe"},
    {"PG_MM_SHORT", &PgKnobs::mmShort, 1, 0, 0, PG_KNOB_ANY, "0: keep the 64-lane lists, no short-list instance (A/B runs)"},
    {"PG_MM_R", &PgKnobs::mmR, 0, 0, 0, PG_KNOB_ANY, "1 / 2 forces 32-row / 64-row passes; present: no gated 32-row alternative"},
    {"PG_MM_SPLIT", &PgKnobs::mmSplit, 1, 0, 0, PG_KNOB_ANY, "0: no column pieces, all rows in plain passes"},
    {"PG_MM_EVICT", &PgKnobs::mmEvict, 1, 0, 0, PG_KNOB_ANY, "0: rows that lose their cap finish inside the pass (no eviction, hence no pieces and no symmetric sweep)"},
    {"PG_MM_PIECES", &PgKnobs::mmPieces, 0, 2, 16, PG_KNOB_RANGE, "column pieces per row block (experiments; at most 8 beyond 64 row blocks)"},
    {"PG_MM_PIECES_AHEAD", &PgKnobs::mmPiecesAhead, 1, 0, 0, PG_KNOB_ANY, "0: the pieces always go through the pass counter"},
    {"PG_MM_PLAN", &PgKnobs::mmPlan, 0, 0, 0, PG_KNOB_ANY, "A/B of the pass rule: 2 = round 2's spreading rule everywhere, 1 = the waves-per-SIMD rule for eps too"},
    {"PG_MM_TAIL", &PgKnobs::mmTail, 0, 0, 0, PG_KNOB_ANY, "1: round 2's rule also shrinks the passes of the last round"},
    {"PG_MM_PERSISTENT", &PgKnobs::mmPersistent, 1, 0, 0, PG_KNOB_ANY, "0: one wave per pass instead of persistent waves"},
    {"PG_MM_L1", &PgKnobs::mmL1, PG_MM_DENSE_L1, 0, 0, PG_KNOB_ANY, "NsqParams::mmDenseL1"},
    {"PG_MM_L2", &PgKnobs::mmL2, PG_MM_DENSE_L2, 0, 0, PG_KNOB_ANY, "NsqParams::mmDenseL2"},
    {"PG_MM_RUN", &PgKnobs::mmRun, PG_MM_DIRECT_RUN, 1, PG_KNOB_MAX, PG_KNOB_CLAMP, "NsqParams::mmDirectRun"},
    {"PG_KNN_SYM", &PgKnobs::knnSym, -1, 0, 0, PG_KNOB_ANY, "symmetric kNN sweep: 0 off, 1 forced wherever the MFMA engine runs the short-list kNN"},
    {"PG_KNN_SYM_CAPL", &PgKnobs::symCapL, PG_SYM_MAX_CAPL, 8, PG_SYM_MAX_CAPL, PG_KNOB_CLAMP, "symmetric sweep: delivered keys per row"},
    {"PG_KNN_SYM_PIECE", &PgKnobs::symPiece, 0, 0, 0, PG_KNOB_ANY, "symmetric sweep: fixed piece length in super-tiles (default: guided)"},
    {"PG_KNN_SYM_PIECE_MIN", &PgKnobs::symPieceMin, 32, 4, PG_KNOB_MAX, PG_KNOB_CLAMP, "symmetric sweep: the guided rule's shortest piece"},
    {"PG_KNN_SYM_OCC", &PgKnobs::symOcc, 0, 1, 4, PG_KNOB_RANGE, "symmetric sweep: waves per SIMD the plan counts on"},
    {"PG_KNN_SYM_DELIVER", &PgKnobs::symDeliver, 1, 0, 0, PG_KNOB_ANY, "0: timing experiments, wrong results"},
    {"PG_KNN_SYM_EVICT_LIMIT", &PgKnobs::symEvictLimit, 0, 0, 0, PG_KNOB_WIDE, "evicted rows up to which the sweep's results stand (default: a sixteenth of the rows)"},
    {"PG_KNN_SYM_MERGE_WGS", &PgKnobs::symMergeWgs, 0, 1, PG_KNOB_MAX, PG_KNOB_RANGE, "workgroups of the sweep's merge at most (tests; default and bound: eight a CU)"},
    {"PG_KNN_SYM_MERGE_WINDOW", &PgKnobs::symMergeWindow, 0, 1, 2, PG_KNOB_RANGE, "delivered keys in the window of the merge's rounds: 1 or 2 (tests: the refill runs often; default: four)"},
};

static inline PgKnob pg_knob_parse(const PgKnobSpec &s, const char *text) {
  PgKnob k = {true, s.dflt};
  if (s.rule == PG_KNOB_NAME) {
    k.v = !strcmp(text, "mfma") ? PG_ENGINE_MFMA : (!strcmp(text, "valu") ? PG_ENGINE_VALU : PG_ENGINE_AUTO);
    return k;
  }
  const long long x = s.rule == PG_KNOB_WIDE ? atoll(text) : (long long)atoi(text);
  if (s.rule == PG_KNOB_CLAMP) k.v = x < s.lo ? s.lo : (x > s.hi ? s.hi : x);
  else if (s.rule == PG_KNOB_RANGE) k.v = x >= s.lo && x <= s.hi ? x : s.dflt;
  else k.v = x;
  return k;
}
// env: a block of "NAME=value" strings ending with a null pointer (the process's `environ`; a test's own).  One walk over
// the block - as with getenv, the first entry of a name counts
static inline PgKnobs pg_knobs_read(const char *const *env) {
  PgKnobs kn;
  for (const PgKnobSpec &s : kPgKnobs) kn.*(s.field) = PgKnob{false, s.dflt};
  for (; env && *env; ++env) {
    const char *e = *env;
    if (e[0] != 'P' || e[1] != 'G' || e[2] != '_') continue;
    const char *eq = strchr(e, '=');
    if (!eq) continue;
    for (const PgKnobSpec &s : kPgKnobs)
      if (strlen(s.name) == (size_t)(eq - e) && !strncmp(s.name, e, (size_t)(eq - e))) {
        if (!(kn.*(s.field)).set) kn.*(s.field) = pg_knob_parse(s, eq + 1);
        break;
      }
  }
  return kn;
}

// =======================================================================================
// Workspace layout.  Launch-private device state of an all-pairs call, sized by the row count:
//   [0, 64)      pass counters of the engine's persistent waves (words 0 and 8: a call's main launch and its gated 32-row
//                alternative) and, word 1, the number of evicted rows                        - zeroed by the call
//   [64, 576)    word 16 (byte 64): the pass counter of the symmetric kNN sweep; word 17: the ticket of its merge's
//                workgroups (the last one decides); the rest reserved - zeroed with the counters
//   [576, 640)   decision words (gates): [0], [1] the probe's (pg_decide_kernel); [2] the word the launches BEHIND a
//                symmetric kNN sweep test (pg_knn_sym_merge_kernel's last workgroup: the probe's gate[0] - 0 without a probe - or 3 =
//                the sweep's results stand, only pg_knn_rows_kernel still runs)
//   [640, ...)   the probe's counts (8 * PG_PROBE_ROWS * PG_PROBE_WAVES bytes)
//   from PG_WS_PARTIAL on, launches of more than PG_SPLIT_MIN_ROWS rows: the lists of the column pieces - at most
//                PG_SPLIT_MAX_ROWS rows x 8 pieces (or half of them x 16) x PG_MM_KL keys; then the evicted rows (below)
// =======================================================================================
#define PG_WS_FLAGS 64
#define PG_WS_GATES 576
#define PG_WS_COUNTS 640
#define PG_WS_PARTIAL (PG_WS_COUNTS + 8 * 64 * 128)
#define PG_SPLIT_MAX_ROWS 8192       // 128 row blocks of 64
#define PG_SPLIT_MIN_ROWS 65536     // (launches up to here never split)
#define PG_SYM_MIN_N 65536          // the symmetric kNN sweep is not chosen below (= PG_PROBE_MIN_N: launches that are probed)
#define PG_WS_PARTIAL_BYTES ((int64_t)PG_SPLIT_MAX_ROWS * 8 * PG_MM_KL * 4)
static_assert(PG_WS_COUNTS + 8 * PG_PROBE_ROWS * PG_PROBE_WAVES <= PG_WS_PARTIAL, "pg_workspace_bytes");
// ... and behind that (every launch) one word per row: the rows a kNN launch of the MFMA engine evicts (NsqParams::mmEvict;
// their number: word 1 of the counter line)
static inline int64_t ws_evict_offset(int64_t nrows) { return PG_WS_PARTIAL + (nrows > PG_SPLIT_MIN_ROWS ? PG_WS_PARTIAL_BYTES : 0); }
static inline int64_t ws_sym_offset(int64_t nrows) { return (ws_evict_offset(nrows) + 4 * (nrows > 0 ? nrows : 0) + 64 + 255) / 256 * 256; }

// ---------------------------------------------------------------------------------------
// The plan of the symmetric kNN sweep (pg_mm_knn_sym_kernel): row block b (64 rows) sweeps the super-tiles from its own,
// b >> 1, to the last one - a triangle of about half the rectangular sweep's visits - and the persistent grid holds one
// wave per slot, so the blocks are cut into PIECES and handed out through the pass counter in block order, longest
// first.  The cut is guided: a block's pieces are about (visits still to hand out) / slots long, at least `pmin` - long
// pieces while there is much left to balance with, short ones at the end, where the waves' finishing times are evened
// out (a fixed length needs ~6 pieces per wave for a makespan within 10 % of the mean; this rule is within 2 % at 200 000
// rows with half as many).  piece > 0: every block in pieces of that length (tests, experiments).  Boundaries inside a
// block fall on even super-tiles (the folded form's tiles are pairs); a piece is at least three super-tiles before
// that rounding, so none is empty.  The same code runs on the host (pg_knn_sym_plan: tests, sizes) and in
// pg_knn_sym_plan_kernel, which writes the plan of a launch into its workspace.
// ---------------------------------------------------------------------------------------
PG_HD static inline int sym_block_pieces(long long b, long long nst, long long slots, int piece, int pmin) {
  const long long len = nst - (b >> 1);
  // visits of the blocks from b on (two blocks per super-tile; a missing last block does not matter to a length rule)
  const long long rem = len * (len + 1) - ((b & 1) ? len : 0);
  long long P = piece > 0 ? piece : (rem / (slots > 0 ? slots : 1)) & ~1ll;
  if (piece <= 0 && P < pmin) P = pmin;
  if (P < 3) P = 3;
  if (P > len) P = len > 3 ? len : 3;
  unsigned np = ((unsigned)len + (unsigned)P - 1u) / (unsigned)P;      // (32-bit: len < 2^17)
  if (np > (unsigned)len / 3u) np = (unsigned)len / 3u;
  if (np > PG_SYM_MAX_PIECES) np = PG_SYM_MAX_PIECES;
  return np < 1 ? 1 : (int)np;
}
// piece q of np of block b: super-tiles [first, end)
PG_HD static inline void sym_piece_range(long long b, long long nst, int np, int q, int *first, int *end) {
  // (32-bit: nst < 2^17 super-tiles at 2^24 columns, np <= 16)
  const unsigned s0 = (unsigned)(b >> 1), len = (unsigned)nst - s0, unp = (unsigned)np, uq = (unsigned)q;
  *first = q == 0 ? (int)s0 : (int)(2u * ((s0 + len * uq / unp + 1u) / 2u));
  *end = q + 1 == np ? (int)nst : (int)(2u * ((s0 + len * (uq + 1u) / unp + 1u) / 2u));
}
static inline long long sym_plan_host(long long n, long long slots, int piece, int pmin, int32_t *out, long long cap) {
  const long long nb = (n + 63) / 64, nst = (n + PG_MM_ST - 1) / PG_MM_ST;
  // the number of passes alone (every call sizes its workspace by it): the last few answers are kept - a walk over all
  // row blocks costs tens of microseconds on the host at 200 000 rows, which a short launch would show
  struct Memo { long long n, slots, count; int piece, pmin; };
  static std::mutex memoLock;
  static Memo memo[4] = {};
  static int memoNext = 0;
  if (!out) {
    std::lock_guard<std::mutex> g(memoLock);
    for (const Memo &m : memo)
      if (m.n == n && m.slots == slots && m.piece == piece && m.pmin == pmin && m.count > 0) return m.count;
  }
  long long at = 0;
  for (long long b = 0; b < nb; ++b) {
    const int np = sym_block_pieces(b, nst, slots, piece, pmin);
    for (int q = 0; q < np; ++q, ++at) {
      if (!out || at >= cap) continue;
      int f, e;
      sym_piece_range(b, nst, np, q, &f, &e);
      out[4 * at] = (int)b; out[4 * at + 1] = f; out[4 * at + 2] = e; out[4 * at + 3] = q;
    }
  }
  if (!out) {
    std::lock_guard<std::mutex> g(memoLock);
    memo[memoNext] = Memo{n, slots, at, piece, pmin};
    memoNext = (memoNext + 1) % 4;
  }
  return at;
}
// wave slots the sweep's plan counts on: `occ` waves per SIMD (PG_KNN_SYM_OCC overrides) on every SIMD of `cus` CUs
static inline long long sym_slots(int occ, int cus, const PgKnobs &kn) {
  if (kn.symOcc.v >= 1) occ = (int)kn.symOcc.v;
  return (long long)(cus > 0 ? cus : 256) * 4 * (occ < 1 ? 1 : (occ > 4 ? 4 : occ));
}
// workspace of the symmetric sweep behind ws_sym_offset: plan (16 bytes a pass), pieceStart, lowCount, the passes' lists
// (sized for the most waves per SIMD the instance can hold, PG_MM_KL keys a row), lowKeys.  0: no such launch at n rows
struct SymWs { int64_t plan, pieceStart, lowCount, partial, lowKeys, bytes; long long maxPasses; };
static inline SymWs sym_ws(int64_t n, int cus, const PgKnobs &kn) {
  SymWs w = {0, 0, 0, 0, 0, 0, 0};
  const int env = (int)kn.knnSym.v;
  if (n <= 0 || n > PG_MAX_N_KNN || env == 0 || (env != 1 && n < PG_SYM_MIN_N)) return w;
  auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
  const long long nb = (n + 63) / 64;
  w.maxPasses = sym_plan_host(n, sym_slots(4, cus, kn), (int)kn.symPiece.v, (int)kn.symPieceMin.v, nullptr, 0);
  w.plan = 0;
  w.pieceStart = up(w.plan + 16 * w.maxPasses);
  w.lowCount = up(w.pieceStart + 4 * (nb + 1));
  w.partial = up(w.lowCount + 4 * n);
  w.lowKeys = up(w.partial + w.maxPasses * 64 * PG_MM_KL * 4);
  w.bytes = up(w.lowKeys + n * (int64_t)kn.symCapL.v * 4);
  return w;
}
// ... and behind the evicted rows, launches the symmetric kNN sweep may take (knn_plan: self graphs from PG_SYM_MIN_N rows
// on): its plan, the lists of its passes and the delivered keys (sym_ws: N x capL x 4 bytes the largest part)
static inline int64_t workspace_bytes(int64_t nrows, int cus, const PgKnobs &kn) { return ws_sym_offset(nrows) + sym_ws(nrows, cus, kn).bytes; }

// =======================================================================================
// The pass planners.  A PassPlan is what a launch of either engine needs of its row split; the executor copies it into
// NsqParams (device code: pg_common.h).
// =======================================================================================
struct PassPlan {
  int rowsPerWave, rowsPerPass;
  long long tailFrom;        // MFMA engine: passes of rowsPerWave rows, the passes from here on have tailRows
  int tailRows;
  long long passes;          // passes (MFMA engine) / waves (VALU engine) in all
  long long gridWaves;
  int grid;                  // workgroups
  int occ;                   // the resident workgroups per CU the plan counted on
};

// waves per CU the VALU engine is sized for under PG_WAVES_PER_CU (multiples of 4)
static inline int waves_per_cu(const PgKnobs &kn) { return (int)(kn.wavesPerCu.v / 4) * 4; }

// VALU engine (pg_nsq.h).  Static, even split of the rows over the waves: every row costs the same (one sweep over all
// columns), so equal row counts are equal work.  The kernel is VALU-issue bound and a workgroup
// puts one wave on each SIMD of its CU, so the run time follows the busiest SIMD:
//     makespan ~ (rows_per_wave + 1) * sum over rounds of T(waves in the round),
//     n = ceil(workgroups / CUs) waves per SIMD run in rounds of `occ` residents (the instance's
//     occupancy), T(1..8) = 2.2, 3.1, 3.7, 4.3, 5.1, 6, 7, 8
// (the +1 is the per-wave cost of streaming the column tiles, ~1 row-equivalent; T(m) reflects
// that fewer than ~5 waves cannot keep the VALU issuing: one wave alone issues under half of the
// time.  Fitted to tools/sweep_rpw.py at N = 50k and 200k, within ~8 %).  rows_per_wave is chosen
// among the multiples of 4 up to one pass (PG_RB) to minimise that; ties go to the larger value
// (fewer column re-reads).  More than PG_RB rows per wave (only with the PG_WAVES_PER_CU /
// PG_ROWS_PER_WAVE overrides) are walked in passes of nearly equal size.
// Second term: every wave streams the whole column matrix (ncols * Q * 16 bytes).  While that fits
// the L2s the stream is hidden; beyond (cfg4: 48 MB) the sweep becomes bound by L2-miss traffic
// served from the Infinity Cache: measured 11.5-15 TB/s aggregate at 48 MB, ~18-20 at 24 MB
// (tools/sweep_rpw_big.py; N = 1M, 125k rows: 16 rows per wave 28.8 ms, 24 rows 20.5 ms).  The plan
// minimises max(VALU makespan, streamed bytes / bandwidth) with bandwidth = 13 TB/s * (48 MB / bytes)^0.65
// (capped at 4x) and 1.21e-11 s per makespan unit and column.
// cus > 0 (the caller refuses a launch without a device)
static inline PassPlan plan_rows(int64_t nrows, int64_t ncols, int cus, int occ, double recBytes, const PgKnobs &kn, int maxRows = PG_RB) {
  long long rpw = 4;
  if (kn.wavesPerCu.set) {
    const long long maxWaves = (long long)cus * waves_per_cu(kn);
    rpw = (nrows + maxWaves - 1) / maxWaves;
    if (rpw < 1) rpw = 1;
    // the filtered sweep takes rows four at a time: whole groups waste no stage-1 work
    if (rpw >= 4) rpw = (rpw + 3) / 4 * 4;
  } else {
    static const long long kRound[9] = {0, 22, 31, 37, 43, 51, 60, 70, 80};   // T(m) x 10
    if (occ < 1) occ = 1;
    if (occ > 8) occ = 8;
    const double matBytes = recBytes * (double)ncols;
    double bw = 13e12;
    if (matBytes > 0 && matBytes < 48e6) bw *= fmin(4.0, pow(48e6 / matBytes, 0.65));
    double best = -1;
    for (long long r = 4; r <= maxRows; r += 4) {
      const long long nw = (nrows + r - 1) / r;
      const long long wgs = (nw + PG_WG_WAVES - 1) / PG_WG_WAVES;
      const long long n = (wgs + cus - 1) / cus;             // waves the busiest SIMD runs
      const double valu = 1.21e-11 * (double)(((n / occ) * kRound[occ] + kRound[n % occ]) * (r + 1));
      const double stream = (double)nw * recBytes / bw;      // both per column
      const double cost = valu > stream ? valu : stream;
      if (best < 0 || cost <= best * 1.0000001) { best = cost; rpw = r; }
    }
  }
  if (kn.rowsPerWave.v > 0) rpw = kn.rowsPerWave.v;          // tuning sweeps
  const long long waves = (nrows + rpw - 1) / rpw;
  const long long passes = (rpw + maxRows - 1) / maxRows;
  PassPlan pl = {};
  pl.occ = occ;
  pl.rowsPerWave = (int)rpw;
  long long rpp = (rpw + passes - 1) / passes;
  if (rpp >= 4) rpp = (rpp + 3) / 4 * 4;
  if (rpp > maxRows) rpp = maxRows;
  pl.rowsPerPass = (int)rpp;
  pl.passes = waves;
  pl.grid = (int)((waves + PG_WG_WAVES - 1) / PG_WG_WAVES);
  pl.gridWaves = (long long)pl.grid * PG_WG_WAVES;
  return pl;
}

// Which all-pairs engine runs a Hamming launch: pg_mm.h (stage 1 on the matrix cores, passes of 32
// rows per wave) or pg_nsq.h (stage 1 on the VALU, 4..32 rows per wave).  PG_ENGINE=mfma / valu forces one.
// Auto: the MFMA engine from 8 waves per SIMD-column on, i.e. once 32-row passes fill the chip; below
// that the VALU engine's finer row split keeps more CUs busy.
static inline bool use_mm_engine(int64_t nrows, const PgKnobs &kn, int l = 64, bool knn = true) {
  if (kn.engine.v == PG_ENGINE_MFMA) return true;
  if (kn.engine.v == PG_ENGINE_VALU) return false;
  // Since the MFMA engine queues its candidates lane-parallel (kNN, and eps slots too: pg_mm.h push_signs) it wins from
  // ~20k rows for kNN (profiles/r03_engine_crossover.txt: N = 16k L = 64 0.24 vs 0.29 ms, L = 32 0.24 vs 0.20) and from
  // ~28k for eps (N = 24k: 0.34 vs 0.27; 32k: 0.41 vs 0.53), ~36k for sequences of one group (L <= 32: only 32 signature
  // bits; N = 50k L = 32 symmetric: 0.43 vs 0.53).  Round 2: 40k / 60k.
  const long long dflt = knn ? 20000 : (l <= 32 ? 36000 : 28000);
  const long long thr = kn.engineMinRows.set ? kn.engineMinRows.v : dflt;
  return nrows >= thr;
}

// MFMA engine (pg_mm.h).  One pass per wave.  A pass takes up to 32 rows (the M of the MFMA tile) and the CU holds 16 waves (four
// workgroups: LDS and VGPR bound), so the grid runs in rounds of `slots` passes.  When 32-row passes would not
// even fill one round, the rows are spread over ~97 % of the slots in smaller passes, down to 16 rows (N=50k L=32
// kNN 1.03 -> 0.90 ms, N=100k L=128 2.40 -> 2.16 ms; tools/rows_sweep.py, profiles/r02_rows_per_pass.txt).
// PG_MM_TAIL=1 also shrinks the passes of the LAST round of a longer grid (tailFrom / tailRows): measured
// slower (dense 200k: 12.5 -> 14.1 ms, cfg3 3.81 -> 3.90) - a round of 2154 full passes on half-empty SIMDs runs
// faster per pass than 3830 passes of 18 rows on full ones - and therefore off.
// PG_ROWS_PER_WAVE = uniform passes of that many rows (tuning sweeps).
// rb: rows per pass of the instance (32 or 64); occ: its resident workgroups per CU (= waves per SIMD).
// Single round (every pass gets a wave slot at once): what a launch takes follows the waves on its busiest SIMD, not the
// rows per wave - every wave streams all column fragments through the matrix pipe whatever its row count (measured at
// 200 000 columns, tools/dbg/balance*.py: one wave per SIMD 0.70 ms, two 0.79, three 0.94, four 1.10-1.14 with 32-row
// passes; 1.26 / 1.52 / 1.87 for two / three / four waves of 64-row passes, the same for 48..64 rows).  So: the fewest
// waves per SIMD that hold the rows, the rows spread evenly over exactly that many waves on every SIMD.  (Round 2 spread
// the rows over ~97 % of ALL slots: 65 536 rows took 1.11 ms as 4096 passes of 16 rows, 0.79 as 2048 of 32.)
static inline PassPlan plan_mm(int64_t nrows, int cus, const PgKnobs &kn, int rb = PG_MM_RB, int occ = 4, bool knn = false, int uniformRows = 0) {
  long long rpw = rb, tailFrom = (nrows + rb - 1) / rb, tailRows = rb;
  const long long simds = (long long)(cus > 0 ? cus : 256) * 4;
  const long long slots = simds * (occ < 1 ? 1 : occ);
  // eps launches keep round 2's spreading rule: their passes are not equal work (symmetric: a pass sweeps the columns
  // above its rows only; matches cost per row) - tools/dbg/plan_ab.py: N = 50k eps <= 2 symmetric 0.58 ms against 0.79
  const int planEnv = (int)kn.mmPlan.v;                                  // (A/B: 2 = round 2's rule, 1 = the new one for eps too)
  const bool oldPlan = planEnv == 2 || (!knn && planEnv != 1);
  if (kn.rowsPerWave.v > 0 || uniformRows > 0) {
    const int want = kn.rowsPerWave.v > 0 ? (int)kn.rowsPerWave.v : uniformRows;
    rpw = want < rb ? want : rb;                            // (a wave sweeps one pass of at most rb rows at a time)
    tailFrom = (nrows + rpw - 1) / rpw; tailRows = rpw;
  } else if (!oldPlan) {
    if (tailFrom <= slots) {
      const long long w = (tailFrom + simds - 1) / simds;               // waves per SIMD
      long long r = (nrows + w * simds - 1) / (w * simds);
      r = (r + 1) / 2 * 2;
      if (r < 4) r = 4;
      if (r > rb) r = rb;
      rpw = r; tailFrom = (nrows + r - 1) / r; tailRows = r;
    }
  } else {
    const long long full = nrows / (slots * rb) * slots;                // passes of the full rounds
    const long long rest = nrows - full * rb;
    if (rest > 0 && (full == 0 || kn.mmTail.v == 1)) {
      long long r = (long long)((double)rest / (0.97 * (double)slots)) + 1;
      r = (r + 1) / 2 * 2;
      if (r < 4) r = 4;
      if (r > rb) r = rb;
      if (full == 0 && r < 16) r = 16;                                  // a single round: at least half-filled MFMA tiles
      tailFrom = full; tailRows = r;
    }
  }
  PassPlan pl = {};
  pl.occ = occ;
  pl.rowsPerWave = (int)rpw; pl.rowsPerPass = rb;
  pl.tailFrom = tailFrom; pl.tailRows = (int)tailRows;
  const long long headRows = tailFrom * rpw < nrows ? tailFrom * rpw : nrows;
  const long long waves = tailFrom + (nrows - headRows + tailRows - 1) / tailRows;
  // persistent waves: at most one per slot of the chip (whole workgroups), the rest of the passes through the counter
  long long gridWaves = waves < slots ? waves : slots;
  if (kn.mmPersistent.v == 0) gridWaves = waves;
  gridWaves = (gridWaves + PG_WG_WAVES - 1) / PG_WG_WAVES * PG_WG_WAVES;
  pl.passes = waves; pl.gridWaves = gridWaves;
  pl.grid = (int)(gridWaves / PG_WG_WAVES);
  return pl;
}

// What a kNN launch of `nrows` rows x `ncols` columns takes (ms) on the 32-row (rb = 32) or the 64-row (rb = 64) short-list
// instance, and which rows go into plain passes (*mainRows; the rest: column pieces, knn_plan).  A round of waves costs
//     T(w, ncols) = S[w] + H[w] * ncols / 100 000,     w = waves on the busiest SIMD
// (it follows the waves per SIMD, not the rows per wave: profiles/r03_pass_plan.txt).  S is what does not grow with the
// columns - the candidates of a row's cluster mates, pass set-up, the tail - H the sweep itself; calibrated at 300 000
// and 900 000 columns of cfg3-like data (tools/dbg/calib.py).  The 64-row instance sweeps twice the rows per fragment
// (H per row 0.6 x) but pays more per pass: 131 072 rows x 200 000 columns 1.07 ms (32-row passes) against 1.27, x
// 1 000 000 columns 4.9 against 3.6 (BASELINE configs[3]: one GPU's 125 000 x 1M block 5.5 -> 3.6 ms).
//   one round   : T(w); with w >= 3 and at most 128 row blocks beyond w - 1 full waves: T(w - 1) + the pieces
//   more rounds : whole rounds of full occupancy + (a last round: T(its waves) | at most 128 row blocks: the pieces)
static inline double knn_plan_cost(long long nrows, long long ncols, int cus, int rb, int occ, bool canSplit, long long *mainRows) {
  static const double S1[4] = {0.43, 0.42, 0.37, 0.12}, H1[4] = {0.148, 0.200, 0.294, 0.477};
  static const double S2[4] = {0.64, 0.69, 0.64, 0.54}, H2[4] = {0.229, 0.292, 0.404, 0.557};
  const bool big = rb > PG_MM_RB;
  const double c = (double)ncols / 1e5, kPieces = 0.04 * c;
  auto T = [&](long long w) { return (big ? S2 : S1)[w - 1] + (big ? H2 : H1)[w - 1] * c; };
  const long long simds = (long long)(cus > 0 ? cus : 256) * 4;
  occ = occ < 1 ? 1 : (occ > 4 ? 4 : occ);
  const long long passes = (nrows + rb - 1) / rb, slots = simds * occ, maxRem = 128ll * rb;
  *mainRows = nrows;
  if (passes <= slots) {
    const long long w = (passes + simds - 1) / simds;
    if (canSplit && w >= 3 && nrows - (w - 1) * simds * rb <= maxRem) {
      *mainRows = (w - 1) * simds * rb;
      return T(w - 1) + kPieces;
    }
    return T(w);
  }
  const long long full = nrows / (slots * rb), rem = nrows - full * slots * rb;
  double t = (double)full * T(occ);
  if (rem > 0) {
    if (canSplit && rem <= maxRem) {
      *mainRows = full * slots * rb;
      t += kPieces;
    } else {
      t += T(((rem + rb - 1) / rb + simds - 1) / simds);
    }
  }
  return t;
}

// PG_PROBE=0: no probe (the size rules alone); neither where an engine is forced
static inline bool probe_enabled(const PgKnobs &kn) { return kn.probe.v != 0 && !kn.engine.set && !kn.engineMinRows.set; }

// =======================================================================================
// The plan of a kNN launch (pg_knn_hamming, pg_knn_hamming_round): every decision, none left to the executor.
// =======================================================================================
struct KnnShape {
  int64_t nrows, ncols, row0;
  bool samePlanes;           // rows and columns are the same packed buffer (with row0 = 0 and nrows = ncols: a self graph)
  int l, bits, k, first;
  bool floorKeys, lastKeys;  // pg_knn_hamming_round's key arrays are given
  bool workspace;
};
struct KnnHw {
  int cus;                   // compute units of the device
  // resident workgroups per CU (= waves per SIMD) of the four instances a launch of this shape may use:
  int occValu;               // pg_nsq_kernel<.., PG_MODE_KNN>
  int occMm32;               // pg_mm_kernel, 32-row passes: the short-list instance where knn_short_list(), else the 64-lane one
  int occMm64;               // pg_mm_kernel, short lists, 64-row passes (unused without short lists)
  int occSym;                // pg_mm_knn_sym_kernel
};
struct KnnPlan {
  bool mm;                   // the MFMA engine (else: one launch of the VALU engine, `valu`)
  uint32_t guess;            // the optimistic stage-1 cap
  uint32_t guessValu;        // ... of the gated VALU launch behind a probe
  bool probe;                // probe + decide + the gated VALU launch run in front
  PassPlan valu;             // the VALU launch (alone, or gated on gate[0] bit 1 behind a probe)
  // --- MFMA engine ---
  bool shortList, two;       // the short-list instance; with 64-row passes
  int mode, rb;              // launcher code and rows per pass of the main launch
  long long mainRows;        // rows in plain passes; the rest (split) in column pieces
  PassPlan main;             // the plain passes of mainRows rows, as plan_mm gives them
  PassPlan launch;           // what the main launch runs: `main`, with the pieces' passes appended when split
  // gate masks: the launches behind a probe test its gate[0], behind a symmetric sweep gate[2] (PG_WS_GATES); no probe, no sweep: no gate
  uint32_t symGateMask, mainGateMask;   // the symmetric sweep and its merge; the main launch and the pieces' merge
  bool evict;
  int64_t evictOffset;       // the evicted rows' list in the workspace
  int evictGrid;             // workgroups of pg_knn_rows_kernel
  uint32_t evictGateMask;    // pg_knn_rows_kernel: the main launch's mask and, behind a sweep, "its results stand" (3)
  bool split;                // mainRows < nrows
  long long nb;              // row blocks of rb rows in pieces
  int pieces;
  bool piecesAhead;          // the pieces start as waves of their own (else: through the pass counter)
  unsigned pieceMergeGrid;
  bool sym;                  // the symmetric sweep runs in front
  long long symSlots, symPasses, symNb, symNst, symGridWaves, symLimit, symZero4;
  int symPiece, symPieceMin;
  uint32_t symCapL;
  int symRowBits;            // the sender row's field of a delivered entry (sym_row_bits of the cap)
  bool symDeliver;
  unsigned symPlanGrid, symMergeGrid;
  int symMergeWindow;        // delivered keys in the window of the merge's rounds: 4; 1 or 2 by PG_KNN_SYM_MERGE_WINDOW (tests)
  bool symPlanRides;         // behind a probe: the plan's workgroups ride in pg_decide_kernel's launch, no plan launch
  int64_t symBase;          // ws_sym_offset; the regions behind it:
  SymWs symWs;
  bool alt32;                // the gated 32-row alternative (the probe's "one cluster")
  PassPlan alt;
};

// short lists (the usual k): the instance that inserts a whole batch of candidates at once (pg_mm.h, KL).
// PG_MM_SHORT=0 keeps the 64-lane lists (A/B runs)
static inline bool knn_short_list(const KnnShape &s, const PgKnobs &kn) {
  return s.first == 1 && s.k + 1 <= PG_MM_KL && !s.floorKeys && !s.lastKeys && kn.mmShort.v != 0;
}

static inline KnnPlan knn_plan(const KnnShape &s, const KnnHw &hw, const PgKnobs &kn) {
  KnnPlan pl = {};
  const int64_t nrows = s.nrows, ncols = s.ncols;
  const int filter = (int)kn.lbFilter.v, nq = plan_nchunks(s.l, s.bits);
  // optimistic stage-1 cap.  pg_nsq.h: 8 = half of what unrelated sequences show in its 32-bit plane-0 bound.
  // pg_mm.h: 10 with the 54-bit signature (L > 32) - unrelated pairs below it are one in 3e6, kNN time is flat from
  // 7 to 12 on every shape tried (tools/guess_sweep.py) and rows whose k-th distance reaches 9 keep their cap;
  // 7 where the signature is the 32 plane-0 bits of a single group (L <= 32: one in 4e3 at 7, one in 400 at 10)
  pl.mm = use_mm_engine(nrows, kn);
  const uint32_t guessMm = s.l > 32 ? 10u : 7u;
  pl.guessValu = 8u;
  pl.guess = kn.knnGuess.set ? (uint32_t)(int)kn.knnGuess.v : (pl.mm ? guessMm : pl.guessValu);
  if (filter == 0) pl.guess = 0;                           // no stage 1, nothing to cap
  if (hw.cus > 0) pl.valu = plan_rows(nrows, ncols, hw.cus, hw.occValu, 16.0 * nq, kn, PG_RB_KNN);
  if (!pl.mm) return pl;
  // Large launches: the data decide between the engines (pg_probe_kernel): unclustered data -> the VALU engine
  pl.probe = probe_enabled(kn) && ncols >= PG_PROBE_MIN_N && nrows >= PG_PROBE_MIN_N / 2 && filter != 0 && !kn.knnGuess.set;
  pl.shortList = knn_short_list(s, kn);
  // ... with 64 rows per pass (every column fragment feeds two MFMAs: half the vector-memory traffic per pair) where
  // that is the cheaper plan (knn_plan_cost; PG_MM_R=1 / 2 forces either).  5-bit L = 64 at 200 000 columns: 32-row passes
  // up to 131 072 rows (1.14 ms against 1.26) and, the rows beyond one full round in column pieces, up to 135 168 (128 row
  // blocks of 32 more); 64-row passes from 135 169 rows on (147 456: 1.55 / 1.47; 196 608: 1.84 / 1.57); L = 128 (three
  // waves per SIMD) N = 100k: 32-row passes 0.75 against 0.97; byte alphabets (64-row instance: two waves per SIMD): 32-row
  // passes.
  // One wave more on every SIMD for a few rows more costs the launch as much as a full round of them (plan_mm), and
  // so does a last round of the persistent waves that only a few passes are left for.  The rows that whole rounds
  // hold go into plain passes; the few beyond - at most 128 row blocks - are swept in PIECES of the columns (as many
  // pieces as give every SIMD about one wave: short passes, a sixteenth or an eighth of a sweep each), and
  // pg_knn_merge_kernel makes the rows' lists of the pieces'.
  // cfg3 (200 000 rows = 3 x 65 536 + 3 392): three waves per SIMD + 53 row blocks x 16 pieces.  PG_MM_SPLIT=0: off
  const int occ1 = hw.occMm32, occ2 = pl.shortList ? hw.occMm64 : 0;
  const bool evictOn = kn.mmEvict.v != 0;
  const bool canSplit = pl.shortList && s.workspace && evictOn && pl.guess > 0 && ncols >= 65536 && nrows > PG_SPLIT_MIN_ROWS &&
                        !kn.rowsPerWave.set && kn.mmSplit.v != 0;
  long long main1 = nrows, main2 = nrows;
  const double t1 = knn_plan_cost(nrows, ncols, hw.cus, PG_MM_RB, occ1, canSplit, &main1);
  const double t2 = pl.shortList ? knn_plan_cost(nrows, ncols, hw.cus, 2 * PG_MM_RB, occ2, canSplit, &main2) : 1e30;
  pl.two = pl.shortList && t2 < t1;
  if (kn.mmR.set) pl.two = pl.shortList && kn.mmR.v == 2;
  pl.rb = pl.two ? 2 * PG_MM_RB : PG_MM_RB;
  const int occm = pl.two ? occ2 : occ1;
  pl.mode = pl.two ? PG_MODE_KNN_SHORT2 : (pl.shortList ? PG_MODE_KNN_SHORT : PG_MODE_KNN);
  pl.mainRows = pl.two ? main2 : main1;
  // the probe's "one cluster" (gate value 2) goes to the 32-row alternative where one is launched; elsewhere
  // the main launch takes it as well
  pl.alt32 = pl.two && pl.probe && !kn.mmR.set;
  if (pl.probe) pl.mainGateMask = pl.alt32 ? (1u << 0) : ((1u << 0) | (1u << 2));
  pl.main = plan_mm(pl.mainRows, hw.cus, kn, pl.rb, occm, true);
  pl.launch = pl.main;
  // rows that lose their optimistic cap are evicted from their passes and finished by pg_knn_rows_kernel behind the
  // launch (NsqParams::mmEvict; PG_MM_EVICT=0: the second phase inside the pass, as before)
  pl.evict = s.first == 1 && !s.floorKeys && !s.lastKeys && pl.guess > 0 && evictOn;
  pl.evictOffset = ws_evict_offset(nrows);
  const long long rowsCap = (long long)(hw.cus > 0 ? hw.cus : 256) * 8;   // (one workgroup per row, the rows in turns)
  pl.evictGrid = (int)(nrows < rowsCap ? nrows : rowsCap);
  // A self graph on the 64-row instance: every unordered pair ONCE (pg_mm.h KS; the plan above).  The
  // sweep, its merge and a decision run in front of the rectangular launch, which then tests a word of its own: it
  // runs only where the merge evicted more rows than pg_knn_rows_kernel finishes for less than a rectangular sweep
  // costs - a sixteenth of them (one row there is one exact sweep of all columns by a workgroup: 12 500 rows x 200 000
  // columns are 2.5e9 exact distances, ~1.4 ms at the VALU engine's direct-form rate, the price of cfg3's whole step).
  pl.symWs = sym_ws(nrows, hw.cus, kn);
  pl.symBase = ws_sym_offset(nrows);
  const bool sym = pl.shortList && pl.evict && s.bits == PG_BITS_5 && nq <= 3 && s.samePlanes && s.row0 == 0 && nrows == ncols &&
                   filter != 0 && pl.symWs.bytes > 0 && (kn.knnSym.v == 1 || pl.two) &&
                   sym_rows_fit(nrows, pl.guess);            // (a sender row fits its field of a delivered entry: sym_entry)
  const long long symSlots = sym ? sym_slots(hw.occSym, hw.cus, kn) : 0;
  const long long symPasses = sym ? sym_plan_host(nrows, symSlots, (int)kn.symPiece.v, (int)kn.symPieceMin.v, nullptr, 0) : 0;
  // (a plan the workspace was not sized for - it is sized for the most slots the instance can have - is not taken:
  //  the rectangular launch stands on its own)
  pl.sym = sym && symPasses <= pl.symWs.maxPasses;
  if (pl.sym) {
    pl.symSlots = symSlots; pl.symPasses = symPasses;
    pl.symPiece = (int)kn.symPiece.v; pl.symPieceMin = (int)kn.symPieceMin.v;
    pl.symNb = (nrows + 63) / 64; pl.symNst = (nrows + PG_MM_ST - 1) / PG_MM_ST;
    pl.symGateMask = 1u << 0;
    pl.symCapL = (uint32_t)kn.symCapL.v;
    pl.symRowBits = sym_row_bits(pl.guess);
    pl.symDeliver = kn.symDeliver.v != 0;
    pl.symGridWaves = ((pl.symPasses < pl.symSlots ? pl.symPasses : pl.symSlots) + PG_WG_WAVES - 1) / PG_WG_WAVES * PG_WG_WAVES;
    // (lowCount: 256-byte aligned and padded to it, so whole uint4 stay inside)
    pl.symZero4 = (nrows + 3) / 4;
    const long long zeroWgs = (pl.symZero4 + 1023) / 1024 < 64 ? (pl.symZero4 + 1023) / 1024 : 64;
    pl.symPlanGrid = (unsigned)(1 + zeroWgs);
    pl.symLimit = kn.symEvictLimit.set ? kn.symEvictLimit.v : nrows / 16;
    // (PG_KNN_SYM_MERGE_WGS: tests - a few workgroups take the rows of a small graph in turns)
    const long long mergeWgs = (nrows + 4 * PG_WG_WAVES - 1) / (4 * PG_WG_WAVES);
    long long mergeCap = rowsCap;
    if (kn.symMergeWgs.v >= 1 && kn.symMergeWgs.v < mergeCap) mergeCap = kn.symMergeWgs.v;
    pl.symMergeGrid = (unsigned)(mergeWgs < mergeCap ? mergeWgs : mergeCap);
    // (PG_KNN_SYM_MERGE_WINDOW: tests - a narrow window makes the refill, the rounds' cold path, run on ordinary inputs)
    pl.symMergeWindow = kn.symMergeWindow.v >= 1 ? (int)kn.symMergeWindow.v : 4;
    // the plan needs the shape and the workspace alone, and the probe's decision launch is one workgroup on an empty chip
    pl.symPlanRides = pl.probe;
    if (!pl.probe) pl.mainGateMask = (1u << 0) | (1u << 2);
  }
  pl.evictGateMask = pl.mainGateMask | (pl.sym ? 1u << 3 : 0u);
  pl.split = pl.mainRows < nrows;
  if (pl.split) {
    const long long rem = nrows - pl.mainRows, nb = (rem + pl.rb - 1) / pl.rb;
    const long long simds = (long long)(hw.cus > 0 ? hw.cus : 256) * 4;
    int pieces = (int)(simds / nb);                         // (nb <= 128: at least 8; nb * pieces <= 1024 passes = the workspace's share)
    pieces = pieces > 16 ? 16 : (pieces < 2 ? 2 : pieces);
    if (kn.mmPieces.v >= 2 && kn.mmPieces.v <= (nb <= 64 ? 16 : 8)) pieces = (int)kn.mmPieces.v;   // (experiments)
    pl.nb = nb; pl.pieces = pieces;
    // the pieces ride in the main launch: its passes beyond the plain ones, fetched through the counter by the waves
    // that finish first - they run while the slower passes are still at work
    pl.launch.passes = pl.main.passes + nb * pieces;       // (plain passes of rb rows: plan_mm gave whole rounds)
    pl.launch.tailFrom = pl.launch.passes; pl.launch.tailRows = pl.rb;
    // ... or, where the chip has slots left beside the plain passes (one round: a wave per SIMD is free), as waves of
    // their own from the start: short guests at four waves per SIMD instead of a tail of 886 waves on an empty chip
    // (PG_MM_PIECES_AHEAD=0: through the counter)
    pl.piecesAhead = pl.main.passes + nb * pieces <= simds * occm && kn.mmPiecesAhead.v != 0;
    if (pl.piecesAhead) {
      pl.launch.gridWaves = (pl.launch.passes + PG_WG_WAVES - 1) / PG_WG_WAVES * PG_WG_WAVES;
      pl.launch.grid = (int)(pl.launch.gridWaves / PG_WG_WAVES);
    }
    pl.pieceMergeGrid = (unsigned)((rem + 4 * PG_WG_WAVES - 1) / (4 * PG_WG_WAVES));
  }
  // the probe may say "one cluster" (gate 2): the same engine with 32-row passes, launched as a third alternative
  if (pl.alt32) pl.alt = plan_mm(nrows, hw.cus, kn, PG_MM_RB, occ1, true);
  return pl;
}
