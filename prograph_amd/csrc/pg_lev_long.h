// Exact Levenshtein distance beyond one 128-bit pattern word: the block form of Myers' bit-vector recurrence
// (Hyyro 2003) as functions that the kernel of pg_lev_long.hip calls and that a host compiler takes too
// (tests/capi_lev_long runs them under the address and undefined-behaviour sanitizers).
//
// The pattern (an X row, length lb) is cut into blocks of 128 rows; block b keeps the vertical deltas of its rows in
// VP[4] / VN[4] (dword w = rows 32w..32w+31), initially ~0 / 0 (D[i][0] = i).  For a text position the blocks are
// stepped from b = 0 upward; each takes a horizontal delta hin in {-1, 0, +1} at its lowest row - +1 for block 0, because
// D[0][j] - D[0][j-1] = 1, else what the block below hands up - and gives the delta of its top row, hout:
//     Eq  = match vector of the block for the text symbol         xnor + 4 x bitop3 per dword
//     Xv  = Eq | VN
//     Eq |= (hin < 0)                                             bit 0
//     Xh  = (((Eq & VP) + VP) ^ VP) | Eq                          the + carries through the four dwords, not across blocks
//     HP  = VN | ~(Xh | VP);   HN = VP & Xh
//     hout = bit127(HP) - bit127(HN)
//     HP  = (HP << 1) | (hin > 0);   HN = (HN << 1) | (hin < 0)
//     VP  = HN | ~(Xv | HP);   VN = HP & Xv
// and after the last text position  d = la + sum_b popcount(VP_b & rows_b) - popcount(VN_b & rows_b),  rows_b the bits of
// block b below lb.  Bit i depends on lower bits and lower blocks only, so padding rows (token 0, which no text symbol
// equals) and blocks wholly above lb never reach a row that counts.
//
// The deltas between two blocks travel in a pair of 32-bit SHIFT REGISTERS, hp / hn, one pair per 32 text positions:
// a step reads its hin from bit 31, shifts the register left and puts its hout into bit 0.  After 32 steps every bit
// is replaced and position i of the 32 sits at bit 31 - i again, which is where the next block's step i reads it.  Both
// the read and the write are folded into funnel shifts (v_alignbit) the recurrence needs anyway, so a step costs 64
// VALU instructions against the 62 of the one-word kernel.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_LL_HD __host__ __device__ __forceinline__
#else
#define PG_LL_HD inline
#endif

#define PG_LEV_LONG_MAX_L 2048
#define PG_LEV_LONG_BLOCK 128                       // pattern rows per block, text positions per chunk
#define PG_LEV_LONG_MAX_BLOCKS (PG_LEV_LONG_MAX_L / PG_LEV_LONG_BLOCK)

namespace pg_ll {

typedef uint32_t u32;

PG_LL_HD u32 and_xnor(u32 a, u32 b, u32 c) {       // a & ~(b ^ c)
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x90);
#else
  return a & ~(b ^ c);
#endif
}

PG_LL_HD u32 xor_or(u32 a, u32 b, u32 c) {         // (a ^ b) | c
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0xBE);
#else
  return (a ^ b) | c;
#endif
}

PG_LL_HD u32 or_nor(u32 a, u32 b, u32 c) {         // a | ~(b | c)
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0xF1);
#else
  return a | ~(b | c);
#endif
}

PG_LL_HD u32 shl1_in(u32 hi, u32 lo) {             // (hi << 1) | (lo >> 31)
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, 31);
#else
  return (hi << 1) | (lo >> 31);
#endif
}

PG_LL_HD u32 add_carry(u32 a, u32 b, u32 &carry) { // a + b + carry; carry out
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_addc(a, b, carry, &carry);
#else
  const uint64_t s = (uint64_t)a + b + carry;
  carry = (u32)(s >> 32);
  return (u32)s;
#endif
}

// One text position on one block.  P: the block's five bit planes, four dwords each; mk[q]: 0 / ~0 as bit q of the text
// symbol; hp / hn: the shift registers described above (FIRST: block 0, hin = +1, the registers are only written).
template <bool FIRST>
PG_LL_HD void step(const u32 (&P)[5][4], const u32 (&mk)[5], u32 (&VP)[4], u32 (&VN)[4], u32 &hp, u32 &hn) {
  u32 Xv[4], HP[4], HN[4], carry = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int w = 0; w < 4; ++w) {
    u32 Eq = ~(P[0][w] ^ mk[0]);
    Eq = and_xnor(Eq, P[1][w], mk[1]);
    Eq = and_xnor(Eq, P[2][w], mk[2]);
    Eq = and_xnor(Eq, P[3][w], mk[3]);
    Eq = and_xnor(Eq, P[4][w], mk[4]);
    Xv[w] = Eq | VN[w];
    if (!FIRST && w == 0) Eq |= hn >> 31;                         // hin < 0
    const u32 t = add_carry(Eq & VP[w], VP[w], carry);
    const u32 Xh = xor_or(t, VP[w], Eq);
    HP[w] = or_nor(VN[w], Xh, VP[w]);
    HN[w] = VP[w] & Xh;
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int w = 3; w >= 0; --w) {
    u32 hps, hns;
    if (w) {
      hps = shl1_in(HP[w], HP[w - 1]);
      hns = shl1_in(HN[w], HN[w - 1]);
    } else if (FIRST) {
      hps = (HP[0] << 1) | 1u;
      hns = HN[0] << 1;
    } else {
      hps = shl1_in(HP[0], hp);                                   // hin > 0 from bit 31 of the register
      hns = shl1_in(HN[0], hn);
    }
    VP[w] = or_nor(hns, Xv[w], hps);
    VN[w] = hps & Xv[w];
  }
  hp = shl1_in(hp, HP[3]);                                        // hout into bit 0
  hn = shl1_in(hn, HN[3]);
}

// `cnt` (1..32) consecutive text positions from j0 on one block and one register pair.  masks(j, mk) gives the plane
// masks of text position j; position j + 1 is fetched before position j is stepped, so the table behind `masks` holds
// one entry more than the text positions (its content is never used).  LAST: no block above takes the registers.
template <bool FIRST, bool LAST, class M>
PG_LL_HD void segment(const u32 (&P)[5][4], M &masks, int j0, int cnt, u32 (&VP)[4], u32 (&VN)[4], u32 &hp, u32 &hn) {
  u32 cur[5], nxt[5];
  masks(j0, cur);
  int i = 0;
  for (; i + 2 <= cnt; i += 2) {                                  // two positions per trip: the two mask sets swap roles
    masks(j0 + i + 1, nxt);
    step<FIRST>(P, cur, VP, VN, hp, hn);
    masks(j0 + i + 2, cur);
    step<FIRST>(P, nxt, VP, VN, hp, hn);
  }
  if (i < cnt) step<FIRST>(P, cur, VP, VN, hp, hn);
  if (!LAST && cnt < 32) {                                        // a short tail: position 0 back to bit 31
    hp <<= 32 - cnt;
    hn <<= 32 - cnt;
  }
}

// the bits of dword w of block b that stand for pattern rows below lb
PG_LL_HD u32 rows_word(int lb, int b, int w) {
  const int nb = lb - PG_LEV_LONG_BLOCK * b - 32 * w;
  return nb >= 32 ? 0xFFFFFFFFu : (nb <= 0 ? 0u : (1u << nb) - 1u);
}

// block b's share of D[lb][la] - la
PG_LL_HD int readoff(const u32 (&VP)[4], const u32 (&VN)[4], int lb, int b) {
  int d = 0;
  for (int w = 0; w < 4; ++w) {
    const u32 rows = rows_word(lb, b, w);
    d += __builtin_popcount(VP[w] & rows) - __builtin_popcount(VN[w] & rows);
  }
  return d;
}

PG_LL_HD int blocks_of(int width) { return (width + PG_LEV_LONG_BLOCK - 1) / PG_LEV_LONG_BLOCK; }

// the block count the kernel is instantiated at for a pattern of this many blocks: 1, 2, 4, 8 or 16
PG_LL_HD int instance_of(int blocks) { return blocks <= 1 ? 1 : blocks <= 2 ? 2 : blocks <= 4 ? 4 : blocks <= 8 ? 8 : 16; }

}  // namespace pg_ll
