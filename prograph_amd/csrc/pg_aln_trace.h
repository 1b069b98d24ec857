// The canonical alignment of one pair: one row of the three integer tables with its direction
// bits, PG_TR_STRIP columns at a time, and the walk back over those bits.  Plain integer code for host and device alike:
// pg_aln_trace.hip calls it with one pair per lane (strides of 64), the checkers under tests/capi_* compile it for the CPU
// (strides of 1).
//
// One recurrence serves the four modes.  i runs over x, j over y, e = gap, oe = gap_open + gap, T = the score table, or
// MINUS the cost table for the global distance, which turns its minimum into a maximum and leaves every equality test -
// the whole of the tie rule - as it is:
//     E[i][j] = max(E[i-1][j] - e, H[i-1][j] - oe),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - oe),
//     H[i][j] = max(H[i-1][j-1] + T[x_i][y_j], E[i][j], F[i][j])      (local: 0 where that is not positive),
// borders H[i][0] = H[0][j] = 0 (global: H[0][0] = 0, else -(gap_open + k e); fit: H[0][j] as global, H[i][0] = 0),
// E[0][j] = F[i][0] = PG_TR_NEG.  The row is swept in strips of PG_TR_STRIP columns, strip s over all rows before strip
// s + 1, the left edge of a strip handed in and its right edge handed out; up to PG_TR_MAX_L positions that is the one
// strip j0 = 0 with the borders as its left edge.  Cells are int32 at every length: |H| <= 2048 * 255 + 255 and
// PG_TR_NEG = -2^28 sinks by at most 2048 * 255 more, so nothing overflows or meets a true value and no table or penalty
// is excluded - the traceback has no "fits" predicate, unlike the 16-bit scoring kernels.
//
// Direction nibble of cell (i, j), i, j >= 1: bits 0-1 where H comes from (0 local stop, 1 diagonal, 2 E, 3 F; the
// diagonal wins a tie, then E), bit 2 "E[i][j] opened from H[i-1][j]", bit 3 "F[i][j] opened from H[i][j-1]" (open wins
// a tie).  Eight cells to a dword: cell j of row i in bits 4 * ((j-1) & 7) of dir[((i-1) * nd + ((j-1) >> 3)) * ds].
//
// PG_TR_FIT (entered through pg_alignment_fit_trace / _long only): all of y inside any substring of x.
// Row 0 is the global one, column 0 is 0; the end cell is the best H[i][len y], i = 0..len x, ties to the smallest i,
// (0, len y) before any row; the walk stops in state H at j = 0 and leaves the j remaining symbols of y unaligned at i = 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_TR_FN __host__ __device__ __forceinline__
#else
#define PG_TR_FN static inline
#endif

#define PG_TR_GLOBAL 0
#define PG_TR_LOCAL 1
#define PG_TR_SEMIGLOBAL 2
#define PG_TR_FIT 3
#define PG_TR_MAX_L 128
#define PG_TR_NEG (-(1 << 28))
#define PG_TR_STRIP 128                 // columns of one strip: a multiple of 8, no dword in two strips
#define PG_TR_LONG_MAX_L 2048
static_assert(PG_TR_STRIP == PG_TR_MAX_L && PG_TR_STRIP % 8 == 0, "up to PG_TR_MAX_L positions are ONE strip");

// token at position p (from 0) of a sequence in pg_sub_pack's dword order: dword g at tok[g * stride], masked to 0..31
PG_TR_FN int pg_tr_token(const uint32_t *tok, long long stride, int p) {
  return (int)((tok[(long long)(p >> 2) * stride] >> (8 * (p & 3))) & 31u);
}

// last non-zero byte + 1 over the ng dwords of a sequence
PG_TR_FN int pg_tr_length(const uint32_t *tok, long long stride, int ng) {
  int len = 0;
  for (int g = 0; g < ng; ++g) {
    const uint32_t w = tok[(long long)g * stride];
    if (w) len = 4 * g + (w >> 24 ? 4 : w >> 16 ? 3 : w >> 8 ? 2 : 1);
  }
  return len;
}

// the running end cell: local the maximal H, semi-global the best of the last row and column, fit the best of the last column
struct pg_tr_end {
  int best, i, j;
};

// H[0][k]; H[k][0] too in every mode but fit (pg_tr_border_x)
PG_TR_FN int pg_tr_border(int mode, int k, int e, int oe) {
  return ((mode == PG_TR_GLOBAL || mode == PG_TR_FIT) && k) ? -(oe - e) - k * e : 0;
}

// H[k][0]: fit leaves the prefix of x free
PG_TR_FN int pg_tr_border_x(int mode, int k, int e, int oe) { return mode == PG_TR_FIT ? 0 : pg_tr_border(mode, k, e, oe); }

// the end cell before any row; semi-global: H[0][len y], or row 0 = row len x; fit: pg_tr_end0_fit after it
PG_TR_FN void pg_tr_end0(int mode, int lx, int ly, pg_tr_end *end) {
  end->best = 0;
  end->i = mode == PG_TR_GLOBAL ? lx : 0;
  end->j = (mode == PG_TR_GLOBAL || mode == PG_TR_FIT) ? ly : (mode == PG_TR_SEMIGLOBAL && lx) ? ly : 0;
}

// fit's end cell before any row: (0, len y) at H[0][len y]
PG_TR_FN void pg_tr_end0_fit(int ly, int e, int oe, pg_tr_end *end) {
  end->best = pg_tr_border(PG_TR_FIT, ly, e, oe);
  end->i = 0;
  end->j = ly;
}

// A candidate (i, j) of value H, whatever was visited before: a larger value replaces, and so does an equal one of a
// smaller i.  Among equal i the earlier strip has the smaller j and stays: local ties go to the smallest i, then the
// smallest j; semi-global cells (i, len y), i < len x, come before the cells (len x, j), as in the canonical order; the
// initial (0, 0) / (0, len y) is never displaced by an equal value.  Within one strip i only grows and the second arm
// never fires: "only a larger value replaces".  pg_tr_row hands in one candidate per row and strip, the FIRST maximum of
// the row's candidates there: the others, taken in j order before or after it, would not replace it or be replaced by it.
PG_TR_FN void pg_tr_end_take(pg_tr_end *end, int H, int i, int j) {
  if (H > end->best || (H == end->best && i < end->i)) {
    end->best = H;
    end->i = i;
    end->j = j;
  }
}

// row 0 of the strip of columns j0 + 1 .. min(j0 + PG_TR_STRIP, ly): cell j at [(j - j0 - 1) * cs]
PG_TR_FN void pg_tr_row0(int mode, int j0, int ly, int e, int oe, int *colH, int *colE, int cs) {
  const int j1 = ly < j0 + PG_TR_STRIP ? ly : j0 + PG_TR_STRIP;
  for (int j = j0 + 1; j <= j1; ++j) {
    colH[(j - j0 - 1) * cs] = pg_tr_border(mode, j, e, oe);
    colE[(j - j0 - 1) * cs] = PG_TR_NEG;
  }
}

// Row i (1..lx) of that strip: colH / colE hold the strip's cells of row i - 1 on entry and of row i on return; trow =
// T[x_i] (32 ints); ytok / ys the STRIP's y tokens as pg_tr_token reads them (column j at position j - j0 - 1).  left =
// H[i][j0], F = F[i][j0], diag = H[i-1][j0] come in (strip 0: pg_tr_border_x(i), PG_TR_NEG, pg_tr_border_x(i - 1));
// *right_h, *right_f = H, F of the strip's last column go out.  The row's direction dwords go to dir[w * ds],
// w < ceil(ly / 8): the nibble of cell j in dword (j - 1) >> 3, bits 4 * ((j - 1) & 7).
PG_TR_FN void pg_tr_row(int mode, int i, int lx, int ly, int j0, int e, int oe, const int *trow, const uint32_t *ytok, long long ys,
                        int *colH, int *colE, int cs, uint32_t *dir, int ds, pg_tr_end *end, int left, int F, int diag,
                        int *right_h, int *right_f) {
  const int j1 = ly < j0 + PG_TR_STRIP ? ly : j0 + PG_TR_STRIP;
  // The candidates of the end cell: every cell (local; semi-global in row len x), or the one of column len y (semi-global,
  // fit) where this strip holds it - its last cell, taken after the loop.  No branch and no test of j in the cell loop:
  // a lane alone on its SIMD waits for every one of them (profiles/aln_pair_frame_ab.txt).
  const bool every = mode == PG_TR_LOCAL || (mode == PG_TR_SEMIGLOBAL && i == lx);
  const bool lastcol = (mode == PG_TR_SEMIGLOBAL || mode == PG_TR_FIT) && j1 == ly && j1 > j0;
  int best = INT32_MIN, bj = 0;                                             // the first maximum among them in this row
  uint32_t bits = 0, yw = 0;
  for (int j = j0 + 1; j <= j1; ++j) {
    const int t = j - j0 - 1, c = t * cs;                                   // the strip's cell, the strip's token
    if ((t & 3) == 0) yw = ytok[(long long)(t >> 2) * ys];                  // one dword of y per four cells
    const int hup = colH[c], eup = colE[c];
    const int eopen = hup - oe, eext = eup - e, fopen = left - oe, fext = F - e;
    const int E = eopen >= eext ? eopen : eext;
    F = fopen >= fext ? fopen : fext;
    const int D = diag + trow[(yw >> (8 * (t & 3))) & 31u];
    int H = D >= E ? D : E;
    if (F > H) H = F;
    uint32_t nib = (H == D ? 1u : H == E ? 2u : 3u) | (eopen >= eext ? 4u : 0u) | (fopen >= fext ? 8u : 0u);
    if (mode == PG_TR_LOCAL && H <= 0) {
      H = 0;
      nib &= ~3u;
    }
    const bool take = every & (H > best);
    best = take ? H : best;
    bj = take ? j : bj;
    diag = hup;
    colH[c] = H;
    colE[c] = E;
    left = H;
    bits |= nib << (4 * ((j - 1) & 7));
    if ((j & 7) == 0) {
      dir[((j - 1) >> 3) * ds] = bits;
      bits = 0;
    }
  }
  if (j1 & 7) dir[((j1 - 1) >> 3) * ds] = bits;                             // the row's last dword, not full (j0 is a multiple of 8)
  if (lastcol && left > best) {
    best = left;
    bj = j1;
  }
  if (bj) pg_tr_end_take(end, best, i, bj);
  *right_h = left;
  *right_f = F;
}

// The distance of the global mode once the last strip is through: `last` = the *right_h of its last row, which no row gave
// when a sequence is empty
PG_TR_FN int pg_tr_global(int lx, int ly, int e, int oe, int last) {
  return -(lx == 0 ? pg_tr_border(PG_TR_GLOBAL, ly, e, oe) : ly == 0 ? pg_tr_border(PG_TR_GLOBAL, lx, e, oe) : last);
}

// The walk back from the end cell over the direction dwords (dir, nd dwords per row, stride ds), starting in state H.
// Writes the codes (1 pair, 2 x symbol unaligned, 3 y symbol unaligned) in forward order to ops[0 .. n_ops), zeroes
// ops[n_ops .. ldo), and fills head[1..6] = x_begin, x_end, y_begin, y_end, n_ops, identities.  ldo >= lx + ly.  Every
// step moves towards (0, 0) and no cell outside 1..lx x 1..ly is read, whatever the dwords hold.  At most min(ldo, cap)
// codes are written: cap = twice the most positions of the entry, 2 * PG_TR_MAX_L or 2 * PG_TR_LONG_MAX_L.
PG_TR_FN void pg_tr_walk_room(int mode, int lx, int ly, int bi, int bj, const uint32_t *xtok, long long xs, const uint32_t *ytok,
                              long long ys, const uint32_t *dir, int nd, int ds, unsigned char *ops, long long ldo, int cap,
                              int32_t *head) {
  int i = bi, j = bj, n = 0, ident = 0, state = 0;
  const int room = (int)(ldo < cap ? ldo : cap);
  while (n < room) {
    if (state == 0 && (i == 0 || j == 0)) {
      if (mode == PG_TR_GLOBAL) {                                           // the rest of the other sequence, unaligned
        for (; i > 0 && n < room; --i) ops[n++] = 2;
        for (; j > 0 && n < room; --j) ops[n++] = 3;
      }
      if (mode == PG_TR_FIT)                                                // all of y: its rest unaligned; x's prefix is free
        for (; j > 0 && n < room; --j) ops[n++] = 3;
      break;
    }
    if (i < 1 || j < 1 || i > lx || j > ly) break;                          // states E and F leave through H: not reached
    const uint32_t nib = (dir[((long long)(i - 1) * nd + ((j - 1) >> 3)) * ds] >> (4 * ((j - 1) & 7))) & 15u;
    if (state == 0) {
      const uint32_t src = nib & 3u;
      if (src == 0) break;                                                  // local: H[i][j] == 0 (never set otherwise)
      if (src == 1) {
        ops[n++] = 1;
        ident += pg_tr_token(xtok, xs, i - 1) == pg_tr_token(ytok, ys, j - 1);
        --i;
        --j;
      } else {
        state = (int)src - 1;                                               // 1: E, 2: F, the same cell
      }
    } else if (state == 1) {
      ops[n++] = 2;
      if (nib & 4u) state = 0;
      --i;
    } else {
      ops[n++] = 3;
      if (nib & 8u) state = 0;
      --j;
    }
  }
  for (int a = 0, b = n - 1; a < b; ++a, --b) {                             // written backwards: turn round
    const unsigned char t = ops[a];
    ops[a] = ops[b];
    ops[b] = t;
  }
  for (long long k = n; k < ldo; ++k) ops[k] = 0;
  head[1] = i;
  head[2] = bi;
  head[3] = j;
  head[4] = bj;
  head[5] = n;
  head[6] = ident;
}
