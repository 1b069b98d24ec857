// Host-side check of the traceback kernel's routines (prograph_amd/csrc/pg_aln_trace.h: pg_tr_end0, pg_tr_row0, pg_tr_row,
// pg_tr_walk_room) as the instance for up to 128 positions runs them - the single strip j0 = 0 - against a plain DP that
// keeps the three tables whole and walks them by comparing entries - the distance minimising over its costs, no negated
// table, no direction bits.  Every buffer the routines get is a heap block of exactly the size they may touch - the strip's
// len y cells, not one more - so the address sanitizer sees a step outside.  After the random pairs `length_sweep` runs
// every len y 0..128 against ten len x, both ways round, in the four modes (fit included), and the pairs that fill a row
// of ops.  Test infrastructure; no GPU.
#include "pg_aln_trace.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (unsigned)(rng_state >> 11);
}

struct Result {
  int score, xb, xe, yb, ye, n, ident;
  std::vector<unsigned char> ops;
};

static const long long BIG = 1ll << 40;

// the definition, literally
static Result plain(int mode, const int T[32][32], int e, int o, const std::vector<int> &x, const std::vector<int> &y) {
  const int lx = (int)x.size(), ly = (int)y.size();
  const bool mn = mode == PG_TR_GLOBAL;
  auto better = [&](long long a, long long b) { return mn ? std::min(a, b) : std::max(a, b); };
  auto open_term = [&](long long h) { return mn ? h + o + e : h - o - e; };
  auto ext_term = [&](long long g) { return mn ? g + e : g - e; };
  const long long none = mn ? BIG : -BIG;
  std::vector<std::vector<long long>> H(lx + 1, std::vector<long long>(ly + 1, 0)), E(lx + 1, std::vector<long long>(ly + 1, none)), F = E;
  if (mn) {
    for (int j = 1; j <= ly; ++j) H[0][j] = o + (long long)j * e;
    for (int i = 1; i <= lx; ++i) H[i][0] = o + (long long)i * e;
  }
  if (mode == PG_TR_FIT)                                                    // all of y is paid for; x's prefix is free
    for (int j = 1; j <= ly; ++j) H[0][j] = -(o + (long long)j * e);
  for (int i = 1; i <= lx; ++i)
    for (int j = 1; j <= ly; ++j) {
      E[i][j] = better(ext_term(E[i - 1][j]), open_term(H[i - 1][j]));
      F[i][j] = better(ext_term(F[i][j - 1]), open_term(H[i][j - 1]));
      long long h = better(H[i - 1][j - 1] + T[x[i - 1]][y[j - 1]], better(E[i][j], F[i][j]));
      H[i][j] = mode == PG_TR_LOCAL ? std::max(0ll, h) : h;
    }
  int bi = lx, bj = ly;
  if (mode == PG_TR_LOCAL) {
    bi = bj = 0;
    for (int i = 0; i <= lx; ++i)
      for (int j = 0; j <= ly; ++j)
        if (H[i][j] > H[bi][bj]) bi = i, bj = j;
  } else if (mode == PG_TR_SEMIGLOBAL) {
    bi = 0, bj = lx ? ly : 0;
    for (int i = 0; i <= lx; ++i)
      for (int j = 0; j <= ly; ++j)
        if ((i == lx || j == ly) && H[i][j] > H[bi][bj]) bi = i, bj = j;
  } else if (mode == PG_TR_FIT) {
    bi = 0;
    for (int i = 1; i <= lx; ++i)
      if (H[i][ly] > H[bi][ly]) bi = i;
  }
  Result r;
  r.score = (int)H[bi][bj];
  r.ident = 0;
  int i = bi, j = bj, state = 0;
  for (;;) {
    if (state == 0) {
      if (mode == PG_TR_LOCAL && H[i][j] == 0) break;
      if (i == 0 || j == 0) {
        if (mode == PG_TR_GLOBAL) {
          for (; i > 0; --i) r.ops.push_back(2);
          for (; j > 0; --j) r.ops.push_back(3);
        }
        if (mode == PG_TR_FIT)
          for (; j > 0; --j) r.ops.push_back(3);
        break;
      }
      if (H[i][j] == H[i - 1][j - 1] + T[x[i - 1]][y[j - 1]]) {
        r.ops.push_back(1);
        r.ident += x[i - 1] == y[j - 1];
        --i, --j;
      } else {
        state = H[i][j] == E[i][j] ? 1 : 2;
      }
    } else if (state == 1) {
      r.ops.push_back(2);
      if (E[i][j] == open_term(H[i - 1][j])) state = 0;
      --i;
    } else {
      r.ops.push_back(3);
      if (F[i][j] == open_term(H[i][j - 1])) state = 0;
      --j;
    }
  }
  std::reverse(r.ops.begin(), r.ops.end());
  r.xb = i, r.xe = bi, r.yb = j, r.ye = bj, r.n = (int)r.ops.size();
  return r;
}

// one sequence in pg_sub_pack's order at column c of a buffer of `stride` columns, width l
static void pack(std::vector<uint32_t> &buf, long long stride, int c, const std::vector<int> &s) {
  for (size_t p = 0; p < s.size(); ++p) buf[(p >> 2) * stride + c] |= (uint32_t)s[p] << (8 * (p & 3));
}

static int bad = 0;
static long long cells = 0;

// one pair through the routines as the one-strip instance runs them, against `plain`; `more`: ldo beyond len x + len y
static void check_pair(int it, int mode, const int T[32][32], int e, int o, const std::vector<int> &x, const std::vector<int> &y,
                       int more) {
  const int lx = (int)x.size(), ly = (int)y.size();
  const Result want = plain(mode, T, e, o, x, y);
  cells += (long long)lx * ly;

  const int xl = std::max(lx, 1), yl = std::max(ly, 1), xg = (xl + 3) / 4, yg = (yl + 3) / 4, nd = (yl + 7) / 8;
  const long long xs = 3, ys = 5;                                         // columns 1 and 2 of small packed matrices
  std::vector<uint32_t> xbuf(xg * xs, 0), ybuf(yg * ys, 0);
  pack(xbuf, xs, 1, x);
  pack(ybuf, ys, 2, y);
  const uint32_t *xt = xbuf.data() + 1, *yt = ybuf.data() + 2;
  if (pg_tr_length(xt, xs, xg) != lx || pg_tr_length(yt, ys, yg) != ly) { ++bad; printf("length\n"); return; }
  int Tm[32 * 32];
  for (int a = 0; a < 32; ++a)
    for (int b = 0; b < 32; ++b) Tm[a * 32 + b] = mode == PG_TR_GLOBAL ? -T[a][b] : T[a][b];
  std::vector<int> colH(ly, 0x5a5a5a5a), colE(ly, 0x5a5a5a5a);           // the strip's cells, not one more
  std::vector<uint32_t> dir((size_t)std::max(lx, 1) * nd, 0xdeadbeefu);
  pg_tr_end end;
  pg_tr_end0(mode, lx, ly, &end);
  if (mode == PG_TR_FIT) pg_tr_end0_fit(ly, e, o + e, &end);
  pg_tr_row0(mode, 0, ly, e, o + e, colH.data(), colE.data(), 1);
  int last = 0;
  for (int i = 1; i <= lx; ++i) {
    int rf;
    pg_tr_row(mode, i, lx, ly, 0, e, o + e, Tm + 32 * pg_tr_token(xt, xs, i - 1), yt, ys, colH.data(), colE.data(), 1,
              dir.data() + (size_t)(i - 1) * nd, 1, &end, pg_tr_border_x(mode, i, e, o + e), PG_TR_NEG,
              pg_tr_border_x(mode, i - 1, e, o + e), &last, &rf);
  }
  const long long ldo = lx + ly + more;                                   // the least the walk may be given, and a little more
  std::vector<unsigned char> ops(ldo, 0xee);
  int32_t head[8] = {0};
  head[0] = mode == PG_TR_GLOBAL ? pg_tr_global(lx, ly, e, o + e, last) : end.best;
  pg_tr_walk_room(mode, lx, ly, end.i, end.j, xt, xs, yt, ys, dir.data(), nd, 1, ops.data(), ldo, 2 * PG_TR_MAX_L, head);
  bool ok = head[0] == want.score && head[1] == want.xb && head[2] == want.xe && head[3] == want.yb && head[4] == want.ye &&
            head[5] == want.n && head[6] == want.ident;
  for (long long k = 0; ok && k < ldo; ++k) ok = ops[k] == (k < want.n ? want.ops[k] : 0);
  if (!ok) {
    ++bad;
    printf("pair %d: mode %d lx %d ly %d e %d o %d: head %d %d %d %d %d %d %d, want %d %d %d %d %d %d %d\n", it, mode, lx, ly, e, o,
           head[0], head[1], head[2], head[3], head[4], head[5], head[6], want.score, want.xb, want.xe, want.yb, want.ye, want.n,
           want.ident);
  }
}

// a sequence of l symbols out of 1..a-1 (symbol 0 inside now and then), ending in a non-zero symbol
static std::vector<int> sequence(int l, int a) {
  std::vector<int> s(l);
  for (int &v : s) v = rnd() % 7 == 0 ? 0 : 1 + rnd() % (a - 1);
  if (l && !s[l - 1]) s[l - 1] = 1;
  return s;
}

// EVERY len y 0..128 against ten len x, both ways round, in the four modes (fit among them), then the pairs that fill a
// row of ops and reach 128 of one kind of column: identical rows, a full row against an empty one, disjoint alphabets under
// cost 255 (all 256 columns are gaps), 128 matches at score 127
static void length_sweep() {
  const int other[10] = {0, 1, 7, 8, 9, 47, 64, 65, 127, 128};
  int T[32][32];
  for (int mode = 0; mode < 4; ++mode) {
    const int A = 6;
    for (int a = 0; a < 32; ++a)
      for (int b = a; b < 32; ++b) {
        int v = 0;
        if (a < A && b < A) v = mode == PG_TR_GLOBAL ? (a == b ? 0 : 1 + (int)(rnd() % 3)) : (a == b ? 1 + (int)(rnd() % 4) : (int)(rnd() % 5) - 3);
        T[a][b] = T[b][a] = v;
      }
    for (int l = 0; l <= PG_TR_MAX_L && bad < 10; ++l)
      for (int k = 0; k < 10; ++k) {
        const int o = (l + k) % 2 ? 11 : 0;
        std::vector<int> a = sequence(l, A), b = sequence(other[k], A);
        if (k % 2 && l && other[k])                                         // related: a long diagonal with a gap in it
          for (int t = 0; t + 1 < std::min(l, other[k]); ++t) b[t] = a[t + (t > l / 2)];
        if (other[k] && !b[other[k] - 1]) b[other[k] - 1] = 1;
        check_pair(100000 + l, mode, T, 2, o, a, b, 0);
        check_pair(200000 + l, mode, T, 2, o, b, a, 0);
      }
  }
  // the extremes
  std::vector<int> full(128), lo(128), hi(128), none;
  for (int t = 0; t < 128; ++t) full[t] = 1 + rnd() % 5, lo[t] = 1 + rnd() % 2, hi[t] = 3 + rnd() % 2;
  for (int mode = 0; mode < 4; ++mode) {
    for (int a = 0; a < 32; ++a)
      for (int b = 0; b < 32; ++b) T[a][b] = mode == PG_TR_GLOBAL ? (a == b ? 0 : 255) : (a == b ? 127 : -128);
    const int pens[3][2] = {{1, 0}, {1, 255}, {255, 255}};
    for (const auto &pen : pens) {
      check_pair(300000 + mode, mode, T, pen[0], pen[1], full, full, 0);
      check_pair(300010 + mode, mode, T, pen[0], pen[1], full, none, 0);
      check_pair(300020 + mode, mode, T, pen[0], pen[1], none, full, 0);
      check_pair(300030 + mode, mode, T, pen[0], pen[1], lo, hi, 0);
      check_pair(300040 + mode, mode, T, pen[0], pen[1], none, none, 0);
    }
  }
}

// without arguments everything; with the argument "sweep" the length sweep alone
int main(int argc, char **argv) {
  const bool only_sweep = argc > 1 && std::string(argv[1]) == "sweep";
  const int gaps[] = {1, 2, 255}, opens[] = {0, 3, 11, 255};
  for (int it = 0; it < 4000 && bad < 10 && !only_sweep; ++it) {
    const int mode = it % 3, A = 2 + rnd() % (it % 7 == 0 ? 30 : 4), e = gaps[rnd() % 3], o = opens[rnd() % 4];
    const int top = it % 5 == 0 ? PG_TR_MAX_L : (it % 2 ? 12 : 40);
    int lx = rnd() % (top + 1), ly = rnd() % (top + 1);
    if (it % 11 == 0) lx = top;
    if (it % 13 == 0) ly = top;
    int T[32][32] = {};
    for (int a = 0; a < A; ++a)
      for (int b = a; b < A; ++b) {
        int v = mode == PG_TR_GLOBAL ? (a == b ? 0 : 1 + (int)(rnd() % (it % 4 ? 3 : 255))) : (int)(rnd() % (it % 4 ? 7 : 256)) - (it % 4 ? 3 : 128);
        T[a][b] = T[b][a] = v;
      }
    std::vector<int> x(lx), y(ly);
    for (int &v : x) v = rnd() % A;
    for (int &v : y) v = rnd() % A;
    if (lx && !x[lx - 1]) x[lx - 1] = 1;                                    // a sequence ends in a non-zero symbol
    if (ly && !y[ly - 1]) y[ly - 1] = 1;
    check_pair(it, mode, T, e, o, x, y, it % 3);
  }
  length_sweep();
  if (bad) printf("TRACE ROUTINES WRONG: %d\n", bad);
  else printf("trace routines OK (%lld cells, the length sweep 0..%d among them)\n", cells, PG_TR_MAX_L);
  return bad != 0;
}
