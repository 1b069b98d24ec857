// Host-side check of the traceback's routines (prograph_amd/csrc/pg_aln_trace.h: pg_tr_end0, pg_tr_row0, pg_tr_row,
// pg_tr_end_take, pg_tr_walk_room) swept as pg_aln_trace.hip's long instance sweeps them - strip s over all rows,
// then strip s + 1, one boundary column in between - against the plain full-table DP of tests/capi_trace/trace_check.cpp
// (`plain`, `pack` and the generator are that file's, its main renamed).  Every buffer the routines get is a heap block of
// exactly the size they may touch, so the address sanitizer sees a step outside.  Test infrastructure; no GPU.
#define main trace_check_main
#include "../capi_trace/trace_check.cpp"
#undef main

// one pair through the strip sweep; false (and a line) when any field differs from `plain`
static bool strips(int tag, int mode, const int T[32][32], int e, int o, const std::vector<int> &x, const std::vector<int> &y, int slack) {
  const int lx = (int)x.size(), ly = (int)y.size(), oe = o + e;
  const Result want = plain(mode, T, e, o, x, y);
  const int xl = std::max(lx, 1), yl = std::max(ly, 1), xg = (xl + 3) / 4, yg = (yl + 3) / 4, nd = (yl + 7) / 8;
  const long long xs = 3, ys = 5;                                           // columns 1 and 2 of small packed matrices
  std::vector<uint32_t> xbuf(xg * xs, 0), ybuf(yg * ys, 0);
  pack(xbuf, xs, 1, x);
  pack(ybuf, ys, 2, y);
  const uint32_t *xt = xbuf.data() + 1, *yt = ybuf.data() + 2;
  int Tm[32 * 32];
  for (int a = 0; a < 32; ++a)
    for (int b = 0; b < 32; ++b) Tm[a * 32 + b] = mode == PG_TR_GLOBAL ? -T[a][b] : T[a][b];
  std::vector<uint32_t> dir((size_t)xl * nd, 0xdeadbeefu);
  std::vector<int> bh(lx, 0x5a5a5a5a), bf(lx, 0x5a5a5a5a);                  // the boundary column: H[i][j0], F[i][j0]
  pg_tr_end end;
  pg_tr_end0(mode, lx, ly, &end);
  int last = 0;
  for (int j0 = 0; j0 < ly; j0 += PG_TR_STRIP) {
    const int width = std::min(PG_TR_STRIP, ly - j0);
    std::vector<int> colH(width, 0x5a5a5a5a), colE(width, 0x5a5a5a5a);     // the strip's cells, not one more
    pg_tr_row0(mode, j0, ly, e, oe, colH.data(), colE.data(), 1);
    int diag = pg_tr_border(mode, j0, e, oe);
    for (int i = 1; i <= lx; ++i) {
      const int left = j0 ? bh[i - 1] : pg_tr_border(mode, i, e, oe), fin = j0 ? bf[i - 1] : PG_TR_NEG;
      int rh, rf;
      pg_tr_row(mode, i, lx, ly, j0, e, oe, Tm + 32 * pg_tr_token(xt, xs, i - 1), yt + (j0 >> 2) * ys, ys, colH.data(),
                colE.data(), 1, dir.data() + (size_t)(i - 1) * nd, 1, &end, left, fin, diag, &rh, &rf);
      diag = left;
      last = rh;
      bh[i - 1] = rh;
      bf[i - 1] = rf;
    }
  }
  const long long ldo = lx + ly + slack;                                    // the least the walk may be given, and a little more
  std::vector<unsigned char> ops(ldo, 0xee);
  int32_t head[8] = {0};
  head[0] = mode == PG_TR_GLOBAL ? pg_tr_global(lx, ly, e, oe, last) : end.best;
  pg_tr_walk_room(mode, lx, ly, end.i, end.j, xt, xs, yt, ys, dir.data(), nd, 1, ops.data(), ldo, 2 * PG_TR_LONG_MAX_L, head);
  bool ok = head[0] == want.score && head[1] == want.xb && head[2] == want.xe && head[3] == want.yb && head[4] == want.ye &&
            head[5] == want.n && head[6] == want.ident;
  for (long long k = 0; ok && k < ldo; ++k) ok = ops[k] == (k < want.n ? want.ops[k] : 0);
  if (!ok)
    printf("pair %d: mode %d lx %d ly %d e %d o %d: head %d %d %d %d %d %d %d, want %d %d %d %d %d %d %d\n", tag, mode, lx, ly, e, o,
           head[0], head[1], head[2], head[3], head[4], head[5], head[6], want.score, want.xb, want.xe, want.yb, want.ye, want.n,
           want.ident);
  return ok;
}

int main() {
  int bad = 0;
  long long cells = 0;
  const int gaps[] = {1, 2, 255}, opens[] = {0, 3, 11, 255};
  const int edges[] = {0, 1, 127, 128, 129, 130, 135, 136, 137, 255, 256, 257, 300};   // around the strips and their dwords
  for (int it = 0; it < 3000 && bad < 10; ++it) {
    const int mode = it % 3, A = 2 + rnd() % (it % 7 == 0 ? 30 : 4), e = gaps[rnd() % 3], o = it % 2 ? 0 : opens[rnd() % 4];
    int lx = it % 4 == 0 ? rnd() % 301 : it % 4 == 1 ? rnd() % 41 : edges[rnd() % 13];
    int ly = it % 5 == 0 ? rnd() % 301 : it % 5 == 1 ? rnd() % 41 : edges[rnd() % 13];
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
    cells += (long long)lx * ly;
    bad += !strips(it, mode, T, e, o, x, y, it % 3);
  }
  // The cross-strip tie: M pairs with M at cells ..(36, 8), N with N at ..(8, 166), 16 either way; 5 matches nothing.  A
  // strip sweep meets (36, 8) first, in strip 0; the canonical end is the smaller i, (8, 166), in strip 1.
  int S[32][32];
  for (int a = 0; a < 32; ++a)
    for (int b = 0; b < 32; ++b) S[a][b] = a == b && a < 5 ? 2 : -3;
  std::vector<int> M, N, x, y;
  for (int k = 0; k < 4; ++k) M.insert(M.end(), {1, 2}), N.insert(N.end(), {3, 4});
  x = N, y = M;
  x.insert(x.end(), 20, 5), y.insert(y.end(), 150, 5);
  x.insert(x.end(), M.begin(), M.end()), y.insert(y.end(), N.begin(), N.end());
  for (int mode = PG_TR_LOCAL; mode <= PG_TR_SEMIGLOBAL; ++mode)
    for (int o = 0; o <= 11; o += 11) {
      const Result w = plain(mode, S, 1, o, x, y);
      if (w.score != 16 || w.xb != 0 || w.xe != 8 || w.yb != 158 || w.ye != 166) ++bad, printf("the tie case is not what it was made for\n");
      bad += !strips(-1, mode, S, 1, o, x, y, 0);
      bad += !strips(-2, mode, S, 1, o, y, x, 0);
    }
  if (bad) printf("LONG TRACE ROUTINES WRONG: %d\n", bad);
  else printf("long trace routines OK (%lld cells)\n", cells);
  return bad != 0;
}
