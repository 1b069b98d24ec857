// Test infrastructure: the block step, the segment loop, the read-off and the row masks of the long Levenshtein kernel
// (prograph_amd/csrc/pg_lev_long.h) compiled for the host and driven exactly as pg_levenshtein_long_dense_kernel drives
// them - operand blocks of five bit planes, the text in chunks of 128 positions with a mask table of 129 entries, the
// pattern blocks inside, four shift-register pairs between two blocks - at every block count the kernel is instantiated
// for, against a plain Wagner-Fischer written here: boundary lengths up to 2048 in every family, and every text and every
// pattern length 0..260 against a set of lengths.  Built with the address and undefined-behaviour sanitizers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "pg_lev_long.h"

using pg_ll::u32;
typedef std::vector<unsigned char> Seq;

static int wagner_fischer(const Seq &y, const Seq &x) {
  std::vector<int> prev(x.size() + 1), cur(x.size() + 1);
  for (size_t j = 0; j <= x.size(); ++j) prev[j] = (int)j;
  for (size_t i = 1; i <= y.size(); ++i) {
    cur[0] = (int)i;
    for (size_t j = 1; j <= x.size(); ++j)
      cur[j] = std::min(prev[j - 1] + (y[i - 1] != x[j - 1]), std::min(prev[j], cur[j - 1]) + 1);
    prev.swap(cur);
  }
  return prev[x.size()];
}

// pg_lev_long_pack's layout for one sequence: planes[b][q][g], bit i of dword g = bit q of token 128 b + 32 g + i
struct Packed {
  int len, width;
  std::vector<u32> planes;
  const u32 (&block(int b) const)[5][4] { return *reinterpret_cast<const u32(*)[5][4]>(&planes[(size_t)b * 20]); }
};

static Packed pack(const Seq &s, int width) {
  Packed p;
  p.len = (int)s.size();
  p.width = width;
  p.planes.assign((size_t)pg_ll::blocks_of(width) * 20, 0u);
  for (int pos = 0; pos < p.len; ++pos)
    for (int q = 0; q < 5; ++q)
      p.planes[(size_t)(pos / 128) * 20 + q * 4 + (pos % 128) / 32] |= (u32)((s[pos] >> q) & 1) << (pos % 32);
  return p;
}

struct Masks {                                  // the LDS table of one chunk: 128 positions and the spare entry
  u32 m[PG_LEV_LONG_BLOCK + 1][5];
  void operator()(int j, u32 (&mk)[5]) const {
    if (j < 0 || j > PG_LEV_LONG_BLOCK) abort();
    for (int q = 0; q < 5; ++q) mk[q] = m[j][q];
  }
};

template <int NB, int B>
static void blocks(const Packed &x, int nbw, int cnt, Masks &masks, u32 (&VP)[NB][4], u32 (&VN)[NB][4], u32 (&hp)[4], u32 (&hn)[4]) {
  if constexpr (B < NB) {
    if (B >= nbw) return;
    u32 P[5][4];
    if (B < pg_ll::blocks_of(x.width)) memcpy(P, x.block(B), sizeof(P));
    else memset(P, 0, sizeof(P));               // a block the operand does not have: padding rows
    for (int g = 0; g < 4; ++g) {
      const int sc = cnt - 32 * g;
      if (sc > 0) pg_ll::segment<B == 0, B == NB - 1>(P, masks, 32 * g, sc < 32 ? sc : 32, VP[B], VN[B], hp[g], hn[g]);
    }
    blocks<NB, B + 1>(x, nbw, cnt, masks, VP, VN, hp, hn);
  }
}

// one (row, column) of the kernel; nbw = the blocks the "wave" runs (at least those of the pattern)
template <int NB>
static int distance(const Packed &x, const Packed &y, int nbw) {
  const int la = y.len, lb = x.len;
  u32 VP[NB][4], VN[NB][4];
  for (int b = 0; b < NB; ++b)
    for (int w = 0; w < 4; ++w) { VP[b][w] = 0xFFFFFFFFu; VN[b][w] = 0u; }
  Masks masks;
  for (int c0 = 0; c0 < la; c0 += PG_LEV_LONG_BLOCK) {
    const int cnt = la - c0;
    const u32 (&yb)[5][4] = y.block(c0 / PG_LEV_LONG_BLOCK);
    for (int j = 0; j < PG_LEV_LONG_BLOCK; ++j)
      for (int q = 0; q < 5; ++q) masks.m[j][q] = 0u - ((yb[q][j >> 5] >> (j & 31)) & 1u);
    for (int q = 0; q < 5; ++q) masks.m[PG_LEV_LONG_BLOCK][q] = 0xDEADBEEFu;      // fetched, never used
    u32 hp[4] = {0u, 0u, 0u, 0u}, hn[4] = {0u, 0u, 0u, 0u};
    blocks<NB, 0>(x, nbw, cnt, masks, VP, VN, hp, hn);
  }
  int d = la;
  for (int b = 0; b < NB; ++b) d += pg_ll::readoff(VP[b], VN[b], lb, b);
  return d;
}

static int distance_at(int nb, const Packed &x, const Packed &y, int nbw) {
  switch (nb) {
    case 1: return distance<1>(x, y, nbw);
    case 2: return distance<2>(x, y, nbw);
    case 4: return distance<4>(x, y, nbw);
    case 8: return distance<8>(x, y, nbw);
    default: return distance<16>(x, y, nbw);
  }
}

static unsigned long long rng_state = 88172645463325252ull;
static u32 rnd(u32 n) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (u32)((rng_state >> 20) % n);
}

static const int LENS[] = {0, 1, 2, 127, 128, 129, 130, 255, 256, 257, 383, 384, 385, 511, 512, 513,
                           1023, 1024, 1025, 1535, 1537, 2046, 2047, 2048};
static const int NLENS = sizeof(LENS) / sizeof(LENS[0]);
static const int NFAM = 6;
static const char *FAMILY[NFAM] = {"homopolymer", "period2", "period3", "parent pieces", "mutant", "small alphabet"};
static Seq parent;

// the pair (x of lb tokens, y of la tokens) of a family
static void make_pair(int fam, int la, int lb, Seq &x, Seq &y) {
  x.assign(lb, 0);
  y.assign(la, 0);
  switch (fam) {
    case 0:                                                       // Eq all ones: the carry runs through whole blocks
      std::fill(x.begin(), x.end(), 31);
      std::fill(y.begin(), y.end(), 31);
      break;
    case 1:                                                       // y = x shifted by one: negative deltas cross the blocks
      for (int i = 0; i < lb; ++i) x[i] = (i & 1) ? 31 : 16;
      for (int i = 0; i < la; ++i) y[i] = (i & 1) ? 16 : 31;
      break;
    case 2:
      for (int i = 0; i < lb; ++i) x[i] = (unsigned char)("\x07\x18\x1f"[i % 3]);
      for (int i = 0; i < la; ++i) y[i] = (unsigned char)("\x07\x18\x1f"[(i + 2) % 3]);
      break;
    case 3:                                                       // a prefix against a suffix of the one parent
      for (int i = 0; i < lb; ++i) x[i] = parent[i];
      for (int i = 0; i < la; ++i) y[i] = parent[PG_LEV_LONG_MAX_L - la + i];
      break;
    case 4: {                                                     // prefixes, y with edits at the block boundaries
      for (int i = 0; i < lb; ++i) x[i] = parent[i];
      for (int i = 0; i < la; ++i) y[i] = parent[i];
      static const int at[] = {127, 128, 255, 256, 1023, 1024};
      for (int e : at)
        if (e < la) y[e] = (unsigned char)(1 + y[e] % 31);
      if (la > 300) {                                             // a deletion at 127 and an insertion at 256: same length
        y.erase(y.begin() + 127);
        y.insert(y.begin() + 256, (unsigned char)(1 + rnd(31)));
      }
      break;
    }
    default:
      for (int i = 0; i < lb; ++i) x[i] = (unsigned char)(1 + rnd(3));
      for (int i = 0; i < la; ++i) y[i] = (unsigned char)(1 + rnd(3));
  }
}

static long checked = 0, runs = 0;

static int check_pair(int fam, int la, int lb) {
  Seq x, y;
  make_pair(fam, la, lb, x, y);
  const int want = wagner_fischer(y, x);
  if (fam == 0 && want != abs(la - lb)) { printf("FAIL reference: homopolymers %d %d -> %d\n", la, lb, want); return 1; }
  ++checked;
  const int need = pg_ll::blocks_of(lb);
  // the pattern at its own width, at the next multiple of 128 and at the full width; the text at its own width
  const int xw[3] = {std::max(lb, 1), std::max(need, 1) * 128, PG_LEV_LONG_MAX_L};
  const Packed py = pack(y, std::max(la, 1));
  for (int wi = 0; wi < 3; ++wi) {
    const Packed px = pack(x, xw[wi]);
    const int inst = pg_ll::instance_of(pg_ll::blocks_of(xw[wi]));
    static const int NBS[] = {1, 2, 4, 8, 16};
    for (int nb : NBS) {
      const bool big = la > 600 || lb > 600;                      // wider instances and widths: the short pairs
      if (nb < inst || (big && (nb > inst || wi == 1))) continue;
      // the wave runs the pattern's own blocks, or every block of the instance (a longer pattern in another lane)
      const int nbws[2] = {need, nb};
      for (int t = big ? wi / 2 : 0; t < (big ? wi / 2 + 1 : 2); ++t) {
        const int got = distance_at(nb, px, py, nbws[t]);
        ++runs;
        if (got != want) {
          printf("FAIL %s la=%d lb=%d width=%d NB=%d blocks run=%d: got %d, want %d\n", FAMILY[fam], la, lb, xw[wi], nb,
                 nbws[t], got, want);
          return 1;
        }
      }
    }
  }
  return 0;
}

// One pair of the every-length sweep: the pattern at its own width, at every instance that width admits, the wave
// running the pattern's own blocks and every block of the instance.
static int sweep_pair(int fam, int la, int lb) {
  Seq x, y;
  make_pair(fam, la, lb, x, y);
  const int want = wagner_fischer(y, x);
  ++checked;
  const int need = pg_ll::blocks_of(lb);
  const Packed px = pack(x, std::max(lb, 1)), py = pack(y, std::max(la, 1));
  const int inst = pg_ll::instance_of(pg_ll::blocks_of(px.width));
  static const int NBS[] = {1, 2, 4, 8, 16};
  for (int nb : NBS) {
    if (nb < inst) continue;
    const int nbws[2] = {need, nb};
    for (int t = 0; t < 2; ++t) {
      const int got = distance_at(nb, px, py, nbws[t]);
      ++runs;
      if (got != want) {
        printf("FAIL sweep %s la=%d lb=%d width=%d NB=%d blocks run=%d: got %d, want %d\n", FAMILY[fam], la, lb, px.width, nb,
               nbws[t], got, want);
        return 1;
      }
    }
  }
  return 0;
}

int main() {
  parent.resize(PG_LEV_LONG_MAX_L);
  for (auto &t : parent) t = (unsigned char)(1 + rnd(31));
  // the row masks
  for (int lb = 0; lb <= PG_LEV_LONG_MAX_L; ++lb) {
    int bits = 0;
    for (int b = 0; b < PG_LEV_LONG_MAX_BLOCKS; ++b)
      for (int w = 0; w < 4; ++w) {
        const u32 r = pg_ll::rows_word(lb, b, w);
        if (r & (r + 1u)) { printf("FAIL rows_word(%d, %d, %d) is no low mask\n", lb, b, w); return 1; }
        bits += __builtin_popcount(r);
      }
    if (bits != lb) { printf("FAIL rows masks of %d hold %d bits\n", lb, bits); return 1; }
  }
  int big0 = 0;
  while (LENS[big0] < 1000) ++big0;
  // every pair of the lengths up to 513 in every family; the long ones against every length, the families in turn
  for (int i = 0; i < NLENS; ++i)
    for (int j = 0; j < NLENS; ++j) {
      if (i < big0 && j < big0) {
        for (int fam = 0; fam < NFAM; ++fam)
          if (check_pair(fam, LENS[i], LENS[j])) return 1;
      } else if (check_pair((i * 5 + j) % NFAM, LENS[i], LENS[j])) {
        return 1;
      }
    }
  // the closed forms at full length
  for (int fam = 0; fam < NFAM; ++fam)
    if (check_pair(fam, 2048, 2048) || check_pair(fam, 0, 2048) || check_pair(fam, 2048, 0)) return 1;
  // every text length 0..260 against a set of pattern lengths, every pattern length 0..260 against the same set as text
  // lengths: every tail and trip count of segment(), every (dword, bit) of the read-off in the first three blocks
  static const int SWEEP[] = {0, 1, 31, 32, 33, 127, 128, 129, 200, 257};
  int turn = 0;
  for (int l = 0; l <= 260; ++l)
    for (int o : SWEEP) {                                           // the families in turn, each way through all of them
      if (sweep_pair(turn % NFAM, l, o) || sweep_pair((turn + 3) % NFAM, o, l)) return 1;
      ++turn;
    }
  printf("every-length sweep: lengths 0..260 against %d lengths, both ways\n", (int)(sizeof(SWEEP) / sizeof(SWEEP[0])));
  printf("lev_long host check OK: %ld pairs, %ld kernel-order evaluations, block counts 1 2 4 8 16\n", checked, runs);
  return 0;
}
