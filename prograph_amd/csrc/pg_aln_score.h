// The cell loop of the SCORE modes (local, semi-global, fit; up to 128 positions and beyond), once: Gotoh's recurrence under
// max, on unsigned registers with saturating subtractions.  DESIGN.md section 4.27; each mode's file says why the floor that
// saturation puts under its cells is exact and where its result is read.
//     E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
//     H[i][j] = max(H[i-1][j-1] + S[x_i][y_j], E[i][j], F[i][j])
// A cell holds H + Z, E + Z, F + Z with a wave-uniform offset Z >= 0 of the mode's choosing, H and E as the halves of one
// dword, P[j] = H | E << 16; -inf is stored as 0 = -Z.  The profile holds S + bias (bytes), the diagonal term is
// (H + byte) -sat- bias.  Per cell:  t = (diag + byte) -sat- bias;  E = max(E -sat- e, H -sat- (o + e));
// F = max(F -sat- e, left -sat- (o + e));  left = max3(t, E, F); the pair H - o - e, E - e is one v_pk_sub_u16 ... clamp.
// Lanes past their own len x sit out the remaining outer steps (EXEC mask, `i < lx`), the folds with them, so after the
// loop a lane's registers are its row len x.
//
// What a mode K chooses:
//     K::ROW0     ALN_ROW0_Z    H[0][j] = 0: every cell Z (local: Z = 0, and the saturation is the recurrence's zero floor)
//                 ALN_ROW0_FIT  H[0][j] = -(o + j e) at the absolute j = j0 + ..., as a chain of saturating subtractions
//     K::FOLD     ALN_FOLD_ALL      every cell of every step goes into `best`, two cells a max3
//                 ALN_FOLD_LASTCOL  column len y alone: len y is wave-uniform but a run-time value inside the last chunk, so
//                                   the 16 cells of that chunk are and-ed with 16 scalar masks (one of them all ones) first; a
//                                   stored value is unsigned, so a masked-out cell is 0 <= best.  Strips before the last
//                                   fold nothing.
//     K::ROWFOLD  row len x of the strip goes into `best` after the loop
// and the caller: LAST - the strip that holds len y (jl: its index inside the last chunk, 1..16); LONG - a boundary column
// in the workspace, read when j0 > 0 and written unless LAST: one dword H | F << 16 per (outer step, lane), laid out
// [i][thread], so a wave reads and writes one coalesced 256-byte line per step, and a lane reads back only what it wrote.
#pragma once
#include "pg_aln_frame.h"

enum { ALN_ROW0_Z, ALN_ROW0_FIT };
enum { ALN_FOLD_ALL, ALN_FOLD_LASTCOL };

// fit's H[0][j] + Z: Z at j = 0, Z - (o + j e) beyond (0 past the operand's width, where it is padding)
__device__ __forceinline__ u32 aln_fit_row0(u32 Z, u32 o, u32 e, int j) { return j ? aln_sat(Z, o + (u32)j * e) : Z; }

// One strip of 16 * NC cells of one Y row against the lane's X sequence: the whole row in the short kernels (j0 = 0, LAST),
// strip j0 / 128 in the long ones.  Q: the strip's profile; best: the maximum so far (+ Z).  Returns the new maximum.
template <class K, int NC, bool LAST, bool LONG>
__device__ __forceinline__ u32 aln_score_strip(const unsigned char *Q, const AlnX &x, u32 *wsb, int j0, int jl, u32 e, u32 oe, u32 bias,
                                               u32 Z, u32 best) {
  const u32 K2 = oe | (e << 16);
  u32 m[16];                                                              // scalar masks: all ones at len y
#pragma unroll
  for (int t = 0; t < 16; ++t) m[t] = (LAST && jl == t + 1) ? 0xffffffffu : 0u;
  u32 P[16 * NC + 1];                                                     // P[j] = H[j0 + j] | E[j0 + j] << 16, + Z each; P[0]: H alone
  if (K::ROW0 == ALN_ROW0_FIT) {
    P[0] = aln_fit_row0(Z, oe - e, e, j0);                                // row 0: H = -(o + j e), E = -inf
    P[1] = aln_fit_row0(Z, oe - e, e, j0 + 1);
#pragma unroll
    for (int j = 2; j <= 16 * NC; ++j) P[j] = aln_sat(P[j - 1], e);       // a chain: one subtraction a column, 0 stays 0
  } else {
#pragma unroll
    for (int j = 0; j <= 16 * NC; ++j) P[j] = Z;                          // row 0: H = 0, E = -inf
  }
  u32 xw = 0;
  for (int i = 0; i < x.lxmax; ++i) {
    if ((i & 3) == 0) xw = aln_x_word(x, i);
    const u32 a = (xw >> (8 * (i & 3))) & 31u;
    if (i < x.lx) {
      const unsigned char *q = Q + a * ALN_QSTRIDE;
      u32 left = Z, F = 0;                                                // H[i][0] = 0, F[i][0] = -inf
      u32 *bd = LONG ? wsb + (long long)i * ALN_THREADS : nullptr;        // this step's line of the boundary column
      if (LONG && j0) {                                                   // wave-uniform
        const u32 v = bd[x.lane];
        left = v & 0xffffu;
        F = v >> 16;
      }
      u32 diag = P[0];
      P[0] = left;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const uint4 v = *(const uint4 *)(q + 16 * c);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        // the diagonal terms first, from the old column: afterwards every cell is rewritten in place
        u32 T[16];
        T[0] = aln_sat((diag & 0xffffu) + (w[0] & 255u), bias);
#pragma unroll
        for (int t = 1; t < 16; ++t) T[t] = aln_sat((P[16 * c + t] & 0xffffu) + ((w[t >> 2] >> (8 * (t & 3))) & 255u), bias);
        diag = P[16 * c + 16];
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
          u32 h[2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const u32 s = aln_sat2(P[16 * c + t + u + 1], K2);            // H -sat- (o + e) | (E -sat- e) << 16
            const u32 E = max(s & 0xffffu, s >> 16);
            F = max(aln_sat(F, e), aln_sat(left, oe));
            left = max(T[t + u], max(E, F));
            P[16 * c + t + u + 1] = left | (E << 16);
            h[u] = left;
          }
          if (K::FOLD == ALN_FOLD_ALL) best = max(max(best, h[0]), h[1]);
          else if (LAST && c == NC - 1) best = max(max(best, h[0] & m[t]), h[1] & m[t + 1]);      // H[i][len y] alone
        }
      }
      if (LONG && !LAST) bd[x.lane] = left | (F << 16);                   // H[i + 1][j0 + 128] | F[i + 1][j0 + 128] << 16
    }
  }
  if (K::ROWFOLD) {                                                       // cells past len y: at most a folded last-column cell
#pragma unroll
    for (int j = 1; j <= 16 * NC; j += 2) best = max(max(best, P[j] & 0xffffu), P[j + 1] & 0xffffu);
  }
  return best;
}

// The local mode (Smith-Waterman; pg_aln_local.hip says why it is exact), here because two files run it: pg_aln_local.hip up
// to 128 positions, pg_aln_long.hip beyond.  Z = 0, so that saturation is the recurrence's zero floor.
struct AlnLocal : AlnModeBase {
  static constexpr bool SCORE = true, TOP = false, ROWFOLD = false;
  static constexpr int ROW0 = ALN_ROW0_Z, FOLD = ALN_FOLD_ALL;
  u32 e, oe, bias;
  __device__ __forceinline__ AlnLocal(const AlnParams &p) : e(p.gap), oe(p.open + p.gap), bias(p.bias) {}
  __device__ __forceinline__ u32 first(int, int) const { return 0u; }       // nothing to align with
  template <int NC>
  __device__ __forceinline__ u32 row(const unsigned char *q, const AlnX &x, int) const {
    return aln_score_strip<AlnLocal, NC, true, false>(q, x, nullptr, 0, 0, e, oe, bias, 0u, 0u);
  }
  template <int NC, bool LAST>
  __device__ __forceinline__ u32 strip(const unsigned char *q, const AlnX &x, u32 *wsb, int j0, int, u32 best) const {
    return aln_score_strip<AlnLocal, NC, LAST, true>(q, x, wsb, j0, 0, e, oe, bias, 0u, best);
  }
};

// The semi-global mode (pg_aln_semiglobal.hip says why it is exact and where its result is read), here because two files
// run it: pg_aln_semiglobal.hip on tokens, pg_aln_profile.hip on profiles.  Z = min(xl, yl) * top of the operand WIDTHS.
struct AlnSemiglobal : AlnModeBase {
  static constexpr bool SCORE = true, TOP = true, ROWFOLD = true;
  static constexpr int ROW0 = ALN_ROW0_Z, FOLD = ALN_FOLD_LASTCOL;
  u32 e, oe, bias, Z;
  // Z <= 128 * 127 in the short kernel; 2 Z + 255 <= 65 535 is the guarantee of the long entry's caller
  __device__ __forceinline__ AlnSemiglobal(const AlnParams &p)
      : e(p.gap), oe(p.open + p.gap), bias(p.bias), Z((u32)min(p.xl, p.yl) * p.top) {}
  __device__ __forceinline__ u32 first(int, int) const { return Z; }        // H[0][len y] = 0
  // rest = len y - j0 >= 1; its index inside the last chunk is rest - ((rest - 1) & ~15), 1..16
  template <int NC>
  __device__ __forceinline__ u32 row(const unsigned char *q, const AlnX &x, int ly) const {
    return aln_score_strip<AlnSemiglobal, NC, true, false>(q, x, nullptr, 0, ly - ((ly - 1) & ~15), e, oe, bias, Z, Z);
  }
  template <int NC, bool LAST>
  __device__ __forceinline__ u32 strip(const unsigned char *q, const AlnX &x, u32 *wsb, int j0, int rest, u32 best) const {
    return aln_score_strip<AlnSemiglobal, NC, LAST, true>(q, x, wsb, j0, rest - ((rest - 1) & ~15), e, oe, bias, Z, best);
  }
  template <typename OUT>
  __device__ __forceinline__ OUT value(u32 d) const { return (OUT)(d - Z); }
};

// The fit mode (pg_aln_fit.hip says why it is exact and where its result is read), here for the same two reasons.
// Z = o + yl (e + top), yl the WIDTH of the Y operand.
struct AlnFit : AlnModeBase {
  static constexpr bool SCORE = true, TOP = true, ROWFOLD = false;           // row len x is NOT folded: all of y must align
  static constexpr int ROW0 = ALN_ROW0_FIT, FOLD = ALN_FOLD_LASTCOL;
  u32 e, o, bias, Z;
  int obias;
  u32 zr, first_r;                                                          // this row's Z and H[0][len y] (short frame)
  // o + yl (e + 2 top) + 255 <= 65 535: the guarantee of either entry's caller, who tests it on the host
  __device__ __forceinline__ AlnFit(const AlnParams &p)
      : e(p.gap), o(p.open), bias(p.bias), Z(p.open + (u32)p.yl * (p.gap + p.top)), obias(p.obias), zr(0), first_r(0) {}
  __device__ __forceinline__ u32 first(int ly, int) const { return aln_fit_row0(Z, o, e, ly); }      // H[0][len y]; Z for an empty y: 0
  // Row 0 differs from column to column but not from row to row of Y: left to itself the compiler forms all 129 values
  // once, ahead of the loop over the rows, and keeps them alive across it - beyond the 168 registers of three waves per
  // SIMD.  The empty statement makes this row's Z a value of its own, so row 0 is formed where it is used.
  __device__ __forceinline__ void begin_row(int ly) {
    zr = Z;
    asm volatile("" : "+s"(zr));
    first_r = aln_fit_row0(zr, o, e, ly);
  }
  template <int NC>
  __device__ __forceinline__ u32 row(const unsigned char *q, const AlnX &x, int ly) const {
    return aln_score_strip<AlnFit, NC, true, false>(q, x, nullptr, 0, ly - ((ly - 1) & ~15), e, o + e, bias, zr, first_r);
  }
  template <int NC, bool LAST>
  __device__ __forceinline__ u32 strip(const unsigned char *q, const AlnX &x, u32 *wsb, int j0, int rest, u32 best) const {
    return aln_score_strip<AlnFit, NC, LAST, true>(q, x, wsb, j0, rest - ((rest - 1) & ~15), e, o + e, bias, Z, best);
  }
  template <typename OUT>
  __device__ __forceinline__ OUT value(u32 d) const { return (OUT)((int)d - (int)Z + obias); }
};
