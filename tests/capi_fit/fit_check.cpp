// Host-side check of the traceback routines in mode PG_TR_FIT (prograph_amd/csrc/pg_aln_trace.h: all of y within any
// substring of x; pg_tr_end0, pg_tr_row0, pg_tr_row with pg_tr_border_x on the left edge, pg_tr_walk_room).  Each pair
// runs twice: as pg_aln_trace.hip's instance for up to 128 positions runs it (the single strip j0 = 0, buffers of exactly
// len y cells, at most 256 codes) and as its long instance does (strips with a boundary column), and is held against
//   * a BRUTE FORCE on small pairs: every substring of x, every alignment path of all of y against it;
//   * the plain full-table DP with the canonical walk on pairs of up to 300 positions (strips of 128 columns), and the
//     replayed score of the returned codes.
// Hand-made pairs: two equal placements of y in x (the canonical one is the FIRST, the smaller i; their cells lie in the
// LAST strip, met in i order) with an earlier strip that holds a larger H in column 128 - a maximum met first in strip
// order that is not an end cell at all; y longer than x; an empty x; an empty y.
// Every buffer the routines get is a heap block of exactly the size they may touch, so the address sanitizer sees a step
// outside.  Test infrastructure; no GPU, no library.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pg_aln_trace.h"

static unsigned long long seed = 0x9e3779b97f4a7c15ull;
static unsigned rnd() {
  seed ^= seed << 13;
  seed ^= seed >> 7;
  seed ^= seed << 17;
  return (unsigned)(seed >> 11);
}

struct Result {
  int score, xb, xe, yb, ye, n, ident;
  std::vector<unsigned char> ops;
};

static const int NEG = -(1 << 28);

// the best global alignment of a[ai..) with b[bj..), `last` the kind of the column before (0 pair / none, 1 a unaligned, 2 b)
static int walk(const int T[32][32], int e, int o, const std::vector<int> &a, const std::vector<int> &b, size_t i, size_t j, int last) {
  if (i == a.size() && j == b.size()) return 0;
  int best = NEG;
  if (i < a.size() && j < b.size()) best = std::max(best, T[a[i]][b[j]] + walk(T, e, o, a, b, i + 1, j + 1, 0));
  if (i < a.size()) best = std::max(best, -e - (last == 1 ? 0 : o) + walk(T, e, o, a, b, i + 1, j, 1));
  if (j < b.size()) best = std::max(best, -e - (last == 2 ? 0 : o) + walk(T, e, o, a, b, i, j + 1, 2));
  return best;
}

static int brute(const int T[32][32], int e, int o, const std::vector<int> &x, const std::vector<int> &y) {
  int best = walk(T, e, o, {}, y, 0, 0, 0);
  for (size_t a0 = 0; a0 < x.size(); ++a0)
    for (size_t a1 = a0 + 1; a1 <= x.size(); ++a1)
      best = std::max(best, walk(T, e, o, std::vector<int>(x.begin() + a0, x.begin() + a1), y, 0, 0, 0));
  return best;
}

// the full tables and the canonical walk, as the header words them
static Result plain(const int T[32][32], int e, int o, const std::vector<int> &x, const std::vector<int> &y) {
  const int lx = (int)x.size(), ly = (int)y.size(), oe = o + e, W = ly + 1;
  std::vector<int> H((size_t)(lx + 1) * W, 0), E((size_t)(lx + 1) * W, NEG), F((size_t)(lx + 1) * W, NEG);
  for (int j = 1; j <= ly; ++j) H[j] = -(o + j * e);
  for (int i = 1; i <= lx; ++i)
    for (int j = 1; j <= ly; ++j) {
      E[i * W + j] = std::max(E[(i - 1) * W + j] - e, H[(i - 1) * W + j] - oe);
      F[i * W + j] = std::max(F[i * W + j - 1] - e, H[i * W + j - 1] - oe);
      H[i * W + j] = std::max(H[(i - 1) * W + j - 1] + T[x[i - 1]][y[j - 1]], std::max(E[i * W + j], F[i * W + j]));
    }
  int bi = 0;
  for (int i = 1; i <= lx; ++i)
    if (H[i * W + ly] > H[bi * W + ly]) bi = i;                             // ties: the smallest i
  Result r;
  r.score = H[bi * W + ly];
  int i = bi, j = ly, state = 0;
  r.ident = 0;
  while (true) {
    if (state == 0) {
      if (j == 0) break;
      if (i == 0) {
        for (; j > 0; --j) r.ops.push_back(3);
        break;
      }
      if (H[i * W + j] == H[(i - 1) * W + j - 1] + T[x[i - 1]][y[j - 1]]) {
        r.ops.push_back(1);
        r.ident += x[i - 1] == y[j - 1];
        --i, --j;
      } else
        state = H[i * W + j] == E[i * W + j] ? 1 : 2;
    } else if (state == 1) {
      r.ops.push_back(2);
      if (E[i * W + j] == H[(i - 1) * W + j] - oe) state = 0;
      --i;
    } else {
      r.ops.push_back(3);
      if (F[i * W + j] == H[i * W + j - 1] - oe) state = 0;
      --j;
    }
  }
  std::reverse(r.ops.begin(), r.ops.end());
  r.xb = i, r.xe = bi, r.yb = 0, r.ye = ly, r.n = (int)r.ops.size();
  return r;
}

// what the codes are worth on x[xb..xe) and all of y; NEG when they do not use up exactly those
static int replay(const int T[32][32], int e, int o, const std::vector<int> &x, const std::vector<int> &y, int xb, int xe,
                  const unsigned char *ops, int n) {
  int i = xb, j = 0, s = 0, last = 0;
  for (int k = 0; k < n; ++k) {
    if (ops[k] == 1) {
      if (i >= xe || j >= (int)y.size()) return NEG;
      s += T[x[i++]][y[j++]];
    } else if (ops[k] == 2) {
      if (i >= xe) return NEG;
      s -= e + (last == 2 ? 0 : o), ++i;
    } else if (ops[k] == 3) {
      if (j >= (int)y.size()) return NEG;
      s -= e + (last == 3 ? 0 : o), ++j;
    } else
      return NEG;
    last = ops[k];
  }
  return i == xe && j == (int)y.size() ? s : NEG;
}

static void pack(std::vector<uint32_t> &buf, long long stride, int col, const std::vector<int> &s) {
  for (size_t p = 0; p < s.size(); ++p) buf[(p >> 2) * stride + col] |= (uint32_t)s[p] << (8 * (p & 3));
}

static bool same(const char *how, int tag, const int32_t *head, const std::vector<unsigned char> &ops, const Result &want, int lx, int ly) {
  bool ok = head[0] == want.score && head[1] == want.xb && head[2] == want.xe && head[3] == want.yb && head[4] == want.ye &&
            head[5] == want.n && head[6] == want.ident;
  for (size_t k = 0; ok && k < ops.size(); ++k) ok = ops[k] == ((int)k < want.n ? want.ops[k] : 0);
  if (!ok)
    printf("%s pair %d: lx %d ly %d: head %d %d %d %d %d %d %d, want %d %d %d %d %d %d %d\n", how, tag, lx, ly, head[0], head[1], head[2],
           head[3], head[4], head[5], head[6], want.score, want.xb, want.xe, want.yb, want.ye, want.n, want.ident);
  return ok;
}

// one pair through both sweeps; false (and a line) when a field differs
static bool both(int tag, const int T[32][32], int e, int o, const std::vector<int> &x, const std::vector<int> &y, int slack, bool small) {
  const int mode = PG_TR_FIT, lx = (int)x.size(), ly = (int)y.size(), oe = o + e;
  const Result want = plain(T, e, o, x, y);
  bool ok = replay(T, e, o, x, y, want.xb, want.xe, want.ops.data(), want.n) == want.score;
  if (small && brute(T, e, o, x, y) != want.score) ok = false;
  if (!ok) printf("pair %d: the plain DP disagrees with the brute force or its own codes\n", tag);
  const int xl = std::max(lx, 1), yl = std::max(ly, 1), xg = (xl + 3) / 4, yg = (yl + 3) / 4, nd = (yl + 7) / 8;
  const long long xs = 3, ys = 5;                                           // columns 1 and 2 of small packed matrices
  std::vector<uint32_t> xbuf(xg * xs, 0), ybuf(yg * ys, 0);
  pack(xbuf, xs, 1, x);
  pack(ybuf, ys, 2, y);
  const uint32_t *xt = xbuf.data() + 1, *yt = ybuf.data() + 2;
  int Tm[32 * 32];
  for (int a = 0; a < 32; ++a)
    for (int b = 0; b < 32; ++b) Tm[a * 32 + b] = T[a][b];
  const long long ldo = lx + ly + slack;
  if (lx <= PG_TR_MAX_L && ly <= PG_TR_MAX_L) {                             // the one strip of up to 128 positions
    std::vector<uint32_t> dir((size_t)xl * nd, 0xdeadbeefu);
    std::vector<int> colH(ly, 0x5a5a5a5a), colE(ly, 0x5a5a5a5a);           // the strip's cells, not one more
    pg_tr_end end;
    pg_tr_end0(mode, lx, ly, &end);
    pg_tr_end0_fit(ly, e, oe, &end);
    pg_tr_row0(mode, 0, ly, e, oe, colH.data(), colE.data(), 1);
    for (int i = 1; i <= lx; ++i) {
      int rh, rf;
      pg_tr_row(mode, i, lx, ly, 0, e, oe, Tm + 32 * pg_tr_token(xt, xs, i - 1), yt, ys, colH.data(), colE.data(), 1,
                dir.data() + (size_t)(i - 1) * nd, 1, &end, pg_tr_border_x(mode, i, e, oe), PG_TR_NEG,
                pg_tr_border_x(mode, i - 1, e, oe), &rh, &rf);
    }
    std::vector<unsigned char> ops(ldo, 0xee);
    int32_t head[8] = {0};
    head[0] = end.best;
    pg_tr_walk_room(mode, lx, ly, end.i, end.j, xt, xs, yt, ys, dir.data(), nd, 1, ops.data(), ldo, 2 * PG_TR_MAX_L, head);
    ok &= same("row", tag, head, ops, want, lx, ly);
  }
  {                                                                         // the long instance's sweep
    std::vector<uint32_t> dir((size_t)xl * nd, 0xdeadbeefu);
    std::vector<int> bh(lx, 0x5a5a5a5a), bf(lx, 0x5a5a5a5a);                // the boundary column: H[i][j0], F[i][j0]
    pg_tr_end end;
    pg_tr_end0(mode, lx, ly, &end);
    pg_tr_end0_fit(ly, e, oe, &end);
    for (int j0 = 0; j0 < ly; j0 += PG_TR_STRIP) {
      const int width = std::min(PG_TR_STRIP, ly - j0);
      std::vector<int> colH(width, 0x5a5a5a5a), colE(width, 0x5a5a5a5a);   // the strip's cells, not one more
      pg_tr_row0(mode, j0, ly, e, oe, colH.data(), colE.data(), 1);
      int diag = pg_tr_border(mode, j0, e, oe);
      for (int i = 1; i <= lx; ++i) {
        const int left = j0 ? bh[i - 1] : pg_tr_border_x(mode, i, e, oe), fin = j0 ? bf[i - 1] : PG_TR_NEG;
        int rh, rf;
        pg_tr_row(mode, i, lx, ly, j0, e, oe, Tm + 32 * pg_tr_token(xt, xs, i - 1), yt + (j0 >> 2) * ys, ys, colH.data(),
                  colE.data(), 1, dir.data() + (size_t)(i - 1) * nd, 1, &end, left, fin, diag, &rh, &rf);
        diag = left;
        bh[i - 1] = rh;
        bf[i - 1] = rf;
      }
    }
    std::vector<unsigned char> ops(ldo, 0xee);
    int32_t head[8] = {0};
    head[0] = end.best;
    pg_tr_walk_room(mode, lx, ly, end.i, end.j, xt, xs, yt, ys, dir.data(), nd, 1, ops.data(), ldo, 2 * PG_TR_LONG_MAX_L, head);
    ok &= same("strip", tag, head, ops, want, lx, ly);
    ok &= replay(T, e, o, x, y, head[1], head[2], ops.data(), head[5]) == want.score;
  }
  return ok;
}

static void table(int T[32][32], int A, bool wide) {
  for (int a = 0; a < 32; ++a)
    for (int b = 0; b < 32; ++b) T[a][b] = 0;
  for (int a = 0; a < A; ++a)
    for (int b = a; b < A; ++b) T[a][b] = T[b][a] = (int)(rnd() % (wide ? 256 : 7)) - (wide ? 128 : 3);
}

static std::vector<int> sequence(int l, int A) {
  std::vector<int> s(l);
  for (int &v : s) v = rnd() % A;
  if (l && !s[l - 1]) s[l - 1] = 1;                                         // a sequence ends in a non-zero symbol
  return s;
}

int main() {
  int bad = 0;
  long long cells = 0;
  const int gaps[] = {1, 2, 255}, opens[] = {0, 3, 11, 255};
  int T[32][32];
  for (int it = 0; it < 1500 && bad < 10; ++it) {                           // small pairs: the brute force
    const int A = 2 + rnd() % 4, e = gaps[rnd() % 3], o = it % 2 ? 0 : opens[rnd() % 4];
    table(T, A, it % 4 == 0);
    const std::vector<int> x = sequence(rnd() % 7, A), y = sequence(rnd() % 7, A);
    bad += !both(it, T, e, o, x, y, it % 3, true);
  }
  const int edges[] = {0, 1, 127, 128, 129, 130, 135, 136, 137, 255, 256, 257, 300};   // around the strips and their dwords
  for (int it = 0; it < 1200 && bad < 10; ++it) {
    const int A = 2 + rnd() % (it % 7 == 0 ? 30 : 4), e = gaps[rnd() % 3], o = it % 2 ? 0 : opens[rnd() % 4];
    table(T, A, it % 4 == 0);
    const int lx = it % 4 == 0 ? rnd() % 301 : it % 4 == 1 ? rnd() % 41 : edges[rnd() % 13];
    const int ly = it % 5 == 0 ? rnd() % 301 : it % 5 == 1 ? rnd() % 41 : edges[rnd() % 13];
    std::vector<int> x = sequence(lx, A), y = sequence(ly, A);
    if (it % 3 == 0 && ly && lx > ly) std::copy(y.begin(), y.end(), x.begin() + rnd() % (lx - ly + 1));      // x holds y
    cells += (long long)lx * ly;
    bad += !both(10000 + it, T, e, o, x, y, it % 3, false);
  }
  // The hand-made pairs.  y = 128 x symbol 1, then 1 2 3 4 (132 symbols: two strips, the second 4 wide); x holds y twice
  // with 6 between.  Strip 0's last column reaches 128 * 2 = 256 at i = 128 and again at i = 266: the largest H the sweep
  // meets before the last strip, in a column that is no end cell.  The end cells (132, 132) and (270, 132) tie at 264;
  // the canonical one is the first.
  for (int a = 0; a < 32; ++a)
    for (int b = 0; b < 32; ++b) T[a][b] = a == b && a > 0 && a < 6 ? 2 : -3;
  std::vector<int> y(128, 1), x;
  y.insert(y.end(), {1, 2, 3, 4});
  x = y;
  x.insert(x.end(), 6, 5);
  x.insert(x.end(), y.begin(), y.end());
  for (int o = 0; o <= 11; o += 11) {
    const Result w = plain(T, 1, o, x, y);
    if (w.score != 264 || w.xb != 0 || w.xe != 132 || w.n != 132) ++bad, printf("the tie case is not what it was made for\n");
    bad += !both(-1, T, 1, o, x, y, 0, false);
    bad += !both(-2, T, 1, o, y, x, 0, false);                              // y longer than x: most of it unaligned
    bad += !both(-3, T, 1, o, {}, y, 1, false);                             // an empty x: every symbol of y unaligned
    bad += !both(-4, T, 1, o, x, {}, 1, false);                             // an empty y: nothing
    const Result v = plain(T, 1, o, {}, y);
    if (v.score != -(o + 132) || v.n != 132 || v.xe != 0) ++bad, printf("the empty x is not the lower bound\n");
  }
  if (bad) printf("FIT TRACE ROUTINES WRONG: %d\n", bad);
  else printf("fit trace OK (%lld cells)\n", cells);
  return bad != 0;
}
