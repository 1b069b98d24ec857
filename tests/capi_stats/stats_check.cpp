// Host-side check of the statistics kernel's routines (prograph_amd/csrc/pg_aln_stats.h: pg_st_row0, pg_st_row, pg_st_head)
// against the traceback's own (pg_aln_trace.h: pg_tr_row0, pg_tr_row, pg_tr_walk_room): the seven fields of the canonical
// alignment, counted forwards, must be the seven fields the walk back over the direction bits gives.  Exhaustive where
// ties are the rule - every pair of sequences over 2 and 3 symbols at all lengths 0..6 under tables of -1..1 (costs 1..2),
// four modes, gap_open 0 and 1 - then random pairs at the lengths around the dwords and at the ends of the range, with the
// extreme tables among them.  In the random part every buffer is a fresh heap block of exactly the size the routines may
// touch, so the address sanitizer sees a step outside.  Last, `length_sweep`: every len y 0..128 against ten len x, both ways
// round, and the pairs that drive a field of the count word to 128, those against the closed form too.  Test infrastructure;
// no GPU.
#include "pg_aln_stats.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (unsigned)(rng_state >> 11);
}

static void pack(std::vector<uint32_t> &buf, long long stride, int c, const std::vector<int> &s) {
  for (size_t p = 0; p < s.size(); ++p) buf[(p >> 2) * stride + c] |= (uint32_t)s[p] << (8 * (p & 3));
}

static int bad = 0;
static long long pairs_done = 0, cells = 0;

// a block of exactly n elements; `exact` (the random part) takes a fresh heap block, so that the sanitizer sees its end
template <class V> static void block(V &v, size_t n, typename V::value_type fillv, bool exact) {
  if (exact) V().swap(v);
  v.assign(n, fillv);
}

// one pair, both ways; Tm is the table as the kernels hold it (negated costs for the distance)
static void compare(int mode, const int *Tm, int e, int o, const std::vector<int> &x, const std::vector<int> &y, bool exact) {
  const int lx = (int)x.size(), ly = (int)y.size(), oe = o + e;
  const int xg = std::max((lx + 3) / 4, 1), yg = std::max((ly + 3) / 4, 1), nd = std::max((ly + 7) / 8, 1);
  const long long xs = 3, ys = 5;                                           // columns 1 and 2 of small packed matrices
  static std::vector<uint32_t> xbuf, ybuf, dir;
  static std::vector<int> colH, colE;
  static std::vector<unsigned char> ops;
  static std::vector<pg_st_cell> col;
  block(xbuf, xg * xs, 0u, exact);
  block(ybuf, yg * ys, 0u, exact);
  pack(xbuf, xs, 1, x);
  pack(ybuf, ys, 2, y);
  const uint32_t *xt = xbuf.data() + 1, *yt = ybuf.data() + 2;

  int32_t want[8] = {0}, got[8] = {0};
  {                                                                         // the traceback: rows, direction bits, the walk
    block(colH, ly, 0, exact);                                              // the one strip's cells, not one more
    block(colE, ly, 0, exact);
    block(dir, (size_t)std::max(lx, 1) * nd, 0xdeadbeefu, exact);
    pg_tr_end end;
    pg_tr_end0(mode, lx, ly, &end);
    if (mode == PG_TR_FIT) pg_tr_end0_fit(ly, e, oe, &end);
    pg_tr_row0(mode, 0, ly, e, oe, colH.data(), colE.data(), 1);
    int last = 0;
    for (int i = 1; i <= lx; ++i) {
      int rf;
      pg_tr_row(mode, i, lx, ly, 0, e, oe, Tm + 32 * pg_tr_token(xt, xs, i - 1), yt, ys, colH.data(), colE.data(), 1,
                dir.data() + (size_t)(i - 1) * nd, 1, &end, pg_tr_border_x(mode, i, e, oe), PG_TR_NEG,
                pg_tr_border_x(mode, i - 1, e, oe), &last, &rf);
    }
    block(ops, lx + ly, (unsigned char)0xee, exact);
    want[0] = mode == PG_TR_GLOBAL ? pg_tr_global(lx, ly, e, oe, last) : end.best;
    pg_tr_walk_room(mode, lx, ly, end.i, end.j, xt, xs, yt, ys, dir.data(), nd, 1, ops.data(), lx + ly, 2 * PG_TR_MAX_L, want);
  }
  {                                                                         // the statistics: rows with their count words
    block(col, ly + 1, pg_st_cell(), exact);
    pg_tr_end end;
    uint32_t endw;
    pg_st_row0(mode, lx, ly, e, oe, col.data(), 1, &end, &endw);
    for (int i = 1; i <= lx; ++i) {
      const int t = pg_tr_token(xt, xs, i - 1);
      pg_st_row(mode, i, lx, ly, e, oe, Tm + 32 * t, t, yt, ys, col.data(), 1, &end, &endw);
    }
    pg_st_head(mode == PG_TR_GLOBAL ? -col[ly].h : end.best, &end, mode == PG_TR_GLOBAL ? col[ly].wh : endw, got);
  }
  ++pairs_done;
  cells += (long long)lx * ly;
  for (int k = 0; k < 7; ++k)
    if (want[k] != got[k]) {
      if (++bad <= 10)
        printf("mode %d lx %d ly %d e %d o %d: stats %d %d %d %d %d %d %d, trace %d %d %d %d %d %d %d\n", mode, lx, ly, e, o, got[0],
               got[1], got[2], got[3], got[4], got[5], got[6], want[0], want[1], want[2], want[3], want[4], want[5], want[6]);
      return;
    }
}

// every sequence over the symbols 1..a of lengths 0..top (a sequence ends in a non-zero symbol: 0 is left out)
static std::vector<std::vector<int>> all_sequences(int a, int top) {
  std::vector<std::vector<int>> out(1);
  for (size_t done = 0, l = 1; (int)l <= top; ++l) {
    const size_t end = out.size();
    for (size_t k = done; k < end; ++k)
      for (int s = 1; s <= a; ++s) {
        std::vector<int> v = out[k];
        v.push_back(s);
        out.push_back(v);
      }
    done = end;
  }
  return out;
}

static void fill(int *Tm, int mode, int a, int kind) {
  // kind 0: identity-like (score 1 / -1, cost 0 / 1); kind 1: one neutral and one dear pair (score 0, cost 2) among them
  for (int k = 0; k < 32 * 32; ++k) Tm[k] = 0;
  for (int p = 0; p <= a; ++p)
    for (int q = 0; q <= a; ++q) {
      int v;
      if (mode == PG_TR_GLOBAL) v = p == q ? 0 : (kind && p + q == 3 ? 2 : 1);
      else v = p == q ? (kind && p == 2 ? 0 : 1) : (kind && p + q == 3 ? 0 : -1);
      Tm[p * 32 + q] = mode == PG_TR_GLOBAL ? -v : v;
    }
}

// The count words at every length and at their largest values.  EVERY len y 0..128 against ten len x, both ways round, in
// the four modes, against the traceback's routines as above; then the pairs that drive a field of the word to 128 - the
// top field's 128 is the sign bit of the word - against the traceback AND the closed form: identical rows (identities =
// pairs = 128), a full row against an empty one (128 x symbols or 128 y symbols unaligned), disjoint alphabets under cost
// 255 (both at once: n_ops = 256 = len x + len y), 128 matches at score 127.
static int32_t head_of(int mode, const int *Tm, int e, int o, const std::vector<int> &x, const std::vector<int> &y, int k) {
  const int lx = (int)x.size(), ly = (int)y.size(), oe = o + e;
  std::vector<uint32_t> xbuf(std::max((lx + 3) / 4, 1), 0u), ybuf(std::max((ly + 3) / 4, 1), 0u);
  pack(xbuf, 1, 0, x);
  pack(ybuf, 1, 0, y);
  std::vector<pg_st_cell> col(ly + 1);
  pg_tr_end end;
  uint32_t endw;
  int32_t got[8] = {0};
  pg_st_row0(mode, lx, ly, e, oe, col.data(), 1, &end, &endw);
  for (int i = 1; i <= lx; ++i) {
    const int t = pg_tr_token(xbuf.data(), 1, i - 1);
    pg_st_row(mode, i, lx, ly, e, oe, Tm + 32 * t, t, ybuf.data(), 1, col.data(), 1, &end, &endw);
  }
  pg_st_head(mode == PG_TR_GLOBAL ? -col[ly].h : end.best, &end, mode == PG_TR_GLOBAL ? col[ly].wh : endw, got);
  return got[k];
}

static void expect(const char *what, int got, int want) {
  if (got != want && ++bad <= 10) printf("%s: %d, want %d\n", what, got, want);
}

static void length_sweep(int *Tm) {
  const int other[10] = {0, 1, 7, 8, 9, 47, 64, 65, 127, 128}, A = 6;
  for (int mode = 0; mode < 4 && bad < 10; ++mode) {
    for (int k = 0; k < 32 * 32; ++k) Tm[k] = 0;
    for (int p = 0; p < A; ++p)
      for (int q = p; q < A; ++q) {
        const int v = mode == PG_TR_GLOBAL ? (p == q ? 0 : 1 + (int)(rnd() % 3)) : (p == q ? 1 + (int)(rnd() % 4) : (int)(rnd() % 5) - 3);
        Tm[p * 32 + q] = Tm[q * 32 + p] = mode == PG_TR_GLOBAL ? -v : v;
      }
    for (int l = 0; l <= PG_TR_MAX_L; ++l)
      for (int k = 0; k < 10; ++k) {
        std::vector<int> a(l), b(other[k]);
        for (int &v : a) v = rnd() % 7 == 0 ? 0 : 1 + rnd() % (A - 1);
        for (int &v : b) v = rnd() % 7 == 0 ? 0 : 1 + rnd() % (A - 1);
        if (k % 2 && l && other[k])                                         // related: a long diagonal with a gap in it
          for (int t = 0; t + 1 < std::min(l, other[k]); ++t) b[t] = a[t + (t > l / 2)];
        if (l && !a[l - 1]) a[l - 1] = 1;
        if (other[k] && !b[other[k] - 1]) b[other[k] - 1] = 1;
        compare(mode, Tm, 2, (l + k) % 2 ? 11 : 0, a, b, true);
        compare(mode, Tm, 2, (l + k) % 2 ? 11 : 0, b, a, true);
      }
  }
  std::vector<int> full(128), lo(128), hi(128), none;
  for (int t = 0; t < 128; ++t) full[t] = 1 + rnd() % 5, lo[t] = 1 + rnd() % 2, hi[t] = 3 + rnd() % 2;
  const int pens[3][2] = {{1, 0}, {1, 255}, {255, 255}};
  for (int mode = 0; mode < 4; ++mode) {
    for (int p = 0; p < 32; ++p)
      for (int q = 0; q < 32; ++q) Tm[p * 32 + q] = mode == PG_TR_GLOBAL ? (p == q ? 0 : -255) : (p == q ? 127 : -128);
    for (const auto &pen : pens) {
      const int e = pen[0], o = pen[1];
      compare(mode, Tm, e, o, full, full, true);
      compare(mode, Tm, e, o, full, none, true);
      compare(mode, Tm, e, o, none, full, true);
      compare(mode, Tm, e, o, lo, hi, true);
      compare(mode, Tm, e, o, none, none, true);
      expect("identical rows: identities", head_of(mode, Tm, e, o, full, full, 6), 128);
      expect("identical rows: n_ops", head_of(mode, Tm, e, o, full, full, 5), 128);
      expect("identical rows: score", head_of(mode, Tm, e, o, full, full, 0), mode == PG_TR_GLOBAL ? 0 : 128 * 127);
      if (mode == PG_TR_GLOBAL) {
        expect("full x, empty y: n_ops", head_of(mode, Tm, e, o, full, none, 5), 128);
        expect("full x, empty y: x_begin", head_of(mode, Tm, e, o, full, none, 1), 0);
        expect("empty x, full y: n_ops", head_of(mode, Tm, e, o, none, full, 5), 128);
        expect("empty x, full y: y_begin", head_of(mode, Tm, e, o, none, full, 3), 0);
        if (e == 1) {                                                       // 256 gaps at 1 beat 128 mismatches at 255
          expect("disjoint: n_ops", head_of(mode, Tm, e, o, lo, hi, 5), 256);
          expect("disjoint: score", head_of(mode, Tm, e, o, lo, hi, 0), 256 + 2 * o);
          expect("disjoint: identities", head_of(mode, Tm, e, o, lo, hi, 6), 0);
          expect("disjoint: x_begin", head_of(mode, Tm, e, o, lo, hi, 1), 0);
          expect("disjoint: y_begin", head_of(mode, Tm, e, o, lo, hi, 3), 0);
        }
      }
      if (mode == PG_TR_FIT) {
        expect("fit, empty x: n_ops", head_of(mode, Tm, e, o, none, full, 5), 128);
        expect("fit, empty x: score", head_of(mode, Tm, e, o, none, full, 0), -(o + 128 * e));
        expect("fit, empty x: y_begin", head_of(mode, Tm, e, o, none, full, 3), 0);
      }
    }
  }
}

// without arguments everything; with the argument "sweep" the length sweep alone
int main(int argc, char **argv) {
  const bool only_sweep = argc > 1 && std::string(argv[1]) == "sweep";
  int Tm[32 * 32];
  // ---- exhaustive: ties are the rule
  for (int a = 2; a <= 3 && !only_sweep; ++a) {
    const std::vector<std::vector<int>> seqs = all_sequences(a, 6);
    for (int mode = 0; mode < 4; ++mode)
      for (int kind = 0; kind < (a == 2 ? 2 : 1); ++kind) {
        fill(Tm, mode, a, a == 2 ? kind : 1);
        for (int o = 0; o <= 1; ++o)
          for (int e = 1; e <= (a == 2 ? 2 : 1); ++e)
            for (const auto &x : seqs)
              for (const auto &y : seqs) compare(mode, Tm, e, o, x, y, false);
      }
  }
  const long long exhaustive = pairs_done;
  // ---- random pairs at the lengths around the dwords and the ends of the range; every fourth the extreme tables
  const int lens[] = {0, 1, 15, 16, 17, 127, 128}, gaps[] = {1, 2, 255}, opens[] = {0, 1, 11, 255};
  for (int it = 0; it < 2400 && bad < 10 && !only_sweep; ++it) {
    const int mode = it % 4, A = 2 + rnd() % (it % 7 == 0 ? 30 : 3);
    const bool extreme = it % 4 == (it / 4) % 4;
    const int e = extreme ? 255 : gaps[rnd() % 3], o = extreme ? 255 : opens[rnd() % 4];
    const int lx = lens[rnd() % 7], ly = lens[rnd() % 7];
    for (int k = 0; k < 32 * 32; ++k) Tm[k] = 0;
    for (int p = 0; p < A; ++p)
      for (int q = p; q < A; ++q) {
        int v;
        if (mode == PG_TR_GLOBAL) v = p == q ? 0 : (extreme ? 255 : 1 + (int)(rnd() % 2));
        else v = extreme ? (p == q ? 127 : -128) : (int)(rnd() % 3) - 1;
        Tm[p * 32 + q] = Tm[q * 32 + p] = mode == PG_TR_GLOBAL ? -v : v;
      }
    std::vector<int> x(lx), y(ly);
    for (int &v : x) v = rnd() % A;
    for (int &v : y) v = rnd() % A;
    if (it % 3 == 0)                                                        // related sequences: long diagonals, few gaps
      for (int k = 0; k < std::min(lx, ly); ++k)
        if (rnd() % 8) y[k] = x[k];
    if (lx && !x[lx - 1]) x[lx - 1] = 1;
    if (ly && !y[ly - 1]) y[ly - 1] = 1;
    compare(mode, Tm, e, o, x, y, true);
  }
  const long long random = pairs_done - exhaustive;
  length_sweep(Tm);
  if (bad) printf("STATS ROUTINES WRONG: %d\n", bad);
  else
    printf("stats routines OK (%lld exhaustive pairs, %lld random, %lld of the length sweep, %lld cells)\n", exhaustive, random,
           pairs_done - exhaustive - random, cells);
  return bad != 0;
}
