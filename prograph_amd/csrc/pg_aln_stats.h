// The STATISTICS of the canonical alignment of one pair without its columns: the forward recurrence of
// pg_aln_trace.h with, beside every H, E and F, the counts of the path the walk of §4.20 would take back from that cell in
// that state.  No direction bits, no walk, no ops.  Plain integer code for host and device alike: pg_aln_stats.hip calls
// it with one pair per lane (cell stride 64), tests/capi_stats/stats_check.cpp compiles it for the CPU (stride 1) beside
// pg_tr_row + pg_tr_walk_room and compares every field.
//
// A count word is four 8-bit fields in one uint32: identities, pairs, x symbols unaligned, y symbols unaligned.  A word
// describes one real path inside a table of at most 128 x 128 positions, so every field is at most 128 and one 32-bit add
// per step never carries from a field into the next.  The walk's choices, made forwards with the same comparisons:
//     in H at (i, j): the diagonal if H = D, else E if H = E, else F    ->  wH = D chosen ? wH[i-1][j-1] + pair (+ identity)
//                                                                                : E chosen ? wE[i][j] : wF[i][j]
//     in E at (i, j): to H[i-1][j] if the open term wins or ties         ->  wE[i][j] = (open ? wH[i-1][j] : wE[i-1][j]) + xgap
//     F mirrors E along j;  local, H <= 0: the walk stops there          ->  wH = 0
// Borders: global H[0][j] has j y-gaps and H[i][0] i x-gaps (the rest of the other sequence, unaligned); fit H[0][j] has j
// y-gaps and H[i][0] none (x's prefix is free); local and semi-global none.  The end cell's word is taken with
// pg_tr_end's (best, i, j) where a larger value arrives - pg_tr_end_take's rule within one strip - so the ties of the end
// cell are the trace's.
// Then n_ops = pairs + xgaps + ygaps, x_begin = x_end - pairs - xgaps, y_begin = y_end - pairs - ygaps.
#pragma once
#include "pg_aln_trace.h"

#define PG_ST_IDENT 0x00000001u
#define PG_ST_PAIR 0x00000100u
#define PG_ST_XGAP 0x00010000u
#define PG_ST_YGAP 0x01000000u

// cell j of the current row: H, E and their count words; 16 bytes, one 128-bit LDS access on the device
struct __attribute__((aligned(16))) pg_st_cell {
  int h, e;
  uint32_t wh, we;
};

// row 0 of the column, the end cell before any row and its word
PG_TR_FN void pg_st_row0(int mode, int lx, int ly, int e, int oe, pg_st_cell *col, int cs, pg_tr_end *end, uint32_t *endw) {
  const bool paid = mode == PG_TR_GLOBAL || mode == PG_TR_FIT;             // H[0][j]: j symbols of y unaligned
  for (int j = 0; j <= ly; ++j) {
    pg_st_cell c;
    c.h = pg_tr_border(mode, j, e, oe);
    c.e = PG_TR_NEG;
    c.wh = paid ? (uint32_t)j * PG_ST_YGAP : 0u;
    c.we = 0u;
    col[j * cs] = c;
  }
  pg_tr_end0(mode, lx, ly, end);
  *endw = 0u;
  if (mode == PG_TR_FIT) {
    pg_tr_end0_fit(ly, e, oe, end);
    *endw = (uint32_t)ly * PG_ST_YGAP;
  }
}

// Row i (1..lx) of one pair: col holds row i - 1 on entry and row i on return (cell j at [j * cs]); trow = T[x_i] (32 ints,
// negated costs for the global distance), xt = x_i itself, ytok / ys the y sequence as pg_tr_token reads it.  The same
// comparisons, in the same order, as pg_tr_row; the candidates of the end cell arrive in its order.
PG_TR_FN void pg_st_row(int mode, int i, int lx, int ly, int e, int oe, const int *trow, int xt, const uint32_t *ytok, long long ys,
                        pg_st_cell *col, int cs, pg_tr_end *end, uint32_t *endw) {
  int left = pg_tr_border_x(mode, i, e, oe);                               // H[i][0]
  uint32_t wleft = mode == PG_TR_GLOBAL ? (uint32_t)i * PG_ST_XGAP : 0u;
  int diag = col[0].h, F = PG_TR_NEG;
  uint32_t wdiag = col[0].wh, wF = 0u;
  col[0].h = left;
  col[0].wh = wleft;
  // Cell j + 1 of row i - 1 and the table entry of its token are fetched one step ahead of their use, the dword of four
  // y tokens one dword ahead: no LDS read is left in the chain that bounds a step.  The last step fetches its own cell
  // again and uses nothing of it; no dword past the last one of the sequence is read.
  const int lastg = ly ? (ly - 1) >> 2 : 0;
  pg_st_cell next = col[(ly ? 1 : 0) * cs];
  uint32_t yw = ly ? ytok[0] : 0u, ywn = ly ? ytok[(lastg ? 1 : 0) * ys] : 0u;
  int ytn = (int)(yw & 31u);
  int tn = trow[ytn];
  for (int j = 1; j <= ly; ++j) {
    const pg_st_cell up = next;
    const int yt = ytn, tj = tn;
    const uint32_t yahead = ywn;                                            // fetched a step ago or earlier
    const int g = (j >> 2) + 1;                                             // the dword after the one of token j
    next = col[(j < ly ? j + 1 : j) * cs];
    ywn = ytok[(long long)(g < lastg ? g : lastg) * ys];
    yw = (j & 3) == 0 ? yahead : yw;                                        // token j (from 0) belongs to cell j + 1
    ytn = j < ly ? (int)((yw >> (8 * (j & 3))) & 31u) : ytn;
    tn = trow[ytn];
    const int eopen = up.h - oe, eext = up.e - e, fopen = left - oe, fext = F - e;
    const int E = eopen >= eext ? eopen : eext;
    const uint32_t wE = (eopen >= eext ? up.wh : up.we) + PG_ST_XGAP;
    wF = (fopen >= fext ? wleft : wF) + PG_ST_YGAP;
    F = fopen >= fext ? fopen : fext;
    const int D = diag + tj;
    const uint32_t wD = wdiag + PG_ST_PAIR + (yt == xt ? PG_ST_IDENT : 0u);
    int H = D >= E ? D : E;
    if (F > H) H = F;
    uint32_t wH = H == D ? wD : H == E ? wE : wF;
    if (mode == PG_TR_LOCAL && H <= 0) {
      H = 0;
      wH = 0u;
    }
    if ((mode == PG_TR_LOCAL || (mode == PG_TR_SEMIGLOBAL && (i == lx || j == ly)) || (mode == PG_TR_FIT && j == ly)) && H > end->best) {
      end->best = H;
      end->i = i;
      end->j = j;
      *endw = wH;
    }
    diag = up.h;
    wdiag = up.wh;
    pg_st_cell c;
    c.h = H;
    c.e = E;
    c.wh = wH;
    c.we = wE;
    col[j * cs] = c;
    left = H;
    wleft = wH;
  }
}

// head[0..6] from the end cell and its word (global: the word of cell (lx, ly), which the caller reads from the column)
PG_TR_FN void pg_st_head(int score, const pg_tr_end *end, uint32_t w, int32_t *head) {
  const int ident = (int)(w & 255u), pairs = (int)((w >> 8) & 255u), xg = (int)((w >> 16) & 255u), yg = (int)(w >> 24);
  head[0] = score;
  head[1] = end->i - pairs - xg;
  head[2] = end->i;
  head[3] = end->j - pairs - yg;
  head[4] = end->j;
  head[5] = pairs + xg + yg;
  head[6] = ident;
}
