// Exact Levenshtein distance of sequences of up to 2048 positions - BUILD DEFINED like pg_lev.hip's kernels, whose
// definition it keeps: the unit-cost edit distance of the non-zero prefixes of zero-right-padded token rows, tokens
// 1..31.  The recurrence (the block form of Myers' bit-vector algorithm) and its read-off are in pg_lev_long.h.
//
// Operand (pg_lev_long_pack): a row of width l is cut into ceil(l / 128) blocks, each bit-sliced like the 128-bit
// operand of pg_levenshtein_dense: uint4 number (b * 5 + q) * npad + s holds bit q of the tokens 128 b .. 128 b + 127 of
// sequence s.  Block b of a long operand is therefore a short operand, and a row range of a packed matrix is the same
// buffer 16 bytes per row further on.
//
// Kernel (pg_levenshtein_long_dense_kernel<NB>): as the one-word kernel, one X row (the pattern) per lane, the Y row
// the wave-uniform text, a workgroup 256 columns x PG_LEVD_ROWS rows.  The text goes by in chunks of 128 positions on
// the outside: a chunk's per-position plane masks sit in LDS (4 KiB per wave), and inside it the pattern blocks are
// stepped from 0 upward, each over the whole chunk.  What block b hands to block b + 1 for the 128 positions of a
// chunk are two 128-bit vectors per lane, kept in eight VGPRs as four pairs of shift registers (pg_lev_long.h).  The
// VP / VN of all NB blocks stay in VGPRs across the chunks - which is what the template on the block count is for: 8 NB
// registers, indexed at compile time once the block loop is unrolled - and a block's 20 plane dwords are reloaded from
// global memory once per (chunk, block): 80 bytes against about 8000 VALU instructions.  Blocks above the longest
// pattern of the wave are skipped (a wave-uniform test).  The trip counts are the text length and that block count:
// there is no lane-dependent branch.  No workspace.
#include "pg_common.h"
#include "pg_lev_long.h"
#include "../../include/prograph_hip.h"

using pg_ll::blocks_of;

// ---------------------------------------------------------------------------------------
// pack: one thread per sequence
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pg_lev_long_pack_kernel(const unsigned char *__restrict__ tok, long long n, int l,
                                                               long long ld, uint4 *__restrict__ planes, long long npad,
                                                               int *__restrict__ lens, u32 *flags) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= npad) return;
  const int nb = blocks_of(l);
  const unsigned char *row = tok + (s < n ? s : 0) * ld;
  int len = 0;
  u32 bad = 0;
  for (int b = 0; b < nb; ++b) {
    u32 w[5][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u32 acc[5] = {0u, 0u, 0u, 0u, 0u};
      for (int i = 0; i < 32; ++i) {
        const int pos = PG_LEV_LONG_BLOCK * b + 32 * g + i;
        const u32 t = (s < n && pos < l) ? (u32)row[pos] : 0u;
        if (t > 31u) bad = 1u;
        if (t != 0u) {
          if (len != pos) bad = 1u;        // zeros must be trailing padding only
          ++len;
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[q] |= ((t >> q) & 1u) << i;
      }
#pragma unroll
      for (int q = 0; q < 5; ++q) w[q][g] = acc[q];
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) planes[((long long)b * 5 + q) * npad + s] = make_uint4(w[q][0], w[q][1], w[q][2], w[q][3]);
  }
  if (s < n) {
    lens[s] = len;
    if (bad) atomicOr(flags, bad);
  }
}

// ---------------------------------------------------------------------------------------
// dense
// ---------------------------------------------------------------------------------------
struct LevLongParams {
  const uint4 *xPlanes;
  long long xNpad, n;
  const int *xLens;
  int xl;
  const uint4 *yPlanes;
  long long yNpad, m;
  const int *yLens;
  int yl;
  void *out;
  int outBytes;
  long long ldo, colTiles;
};

// blocks B .. nbw - 1 of one chunk (`cnt` text positions left, 128 at most taken), B a compile-time index of VP / VN
template <int NB, int B, class M>
__device__ __forceinline__ void lev_long_blocks(const LevLongParams &p, u32 colOff, int nbw, int cnt, M &masks,
                                                u32 (&VP)[NB][4], u32 (&VN)[NB][4], u32 (&hp)[4], u32 (&hn)[4]) {
  if constexpr (B < NB) {
    if (B >= nbw) return;
    u32 P[5][4];
    // a wave-uniform base and one 32-bit lane offset, formed here: hoisted out of the chunk loop the addresses would
    // cost a VGPR pair per (block, plane), more than VP and VN themselves
    u32 off = colOff;
    asm volatile("" : "+v"(off));
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const uint4 v = *(const uint4 *)((const char *)(p.xPlanes + ((long long)B * 5 + q) * p.xNpad) + off);
      P[q][0] = v.x; P[q][1] = v.y; P[q][2] = v.z; P[q][3] = v.w;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int sc = cnt - 32 * g;
      if (sc > 0) pg_ll::segment<B == 0, B == NB - 1>(P, masks, 32 * g, sc < 32 ? sc : 32, VP[B], VN[B], hp[g], hn[g]);
    }
    lev_long_blocks<NB, B + 1>(p, colOff, nbw, cnt, masks, VP, VN, hp, hn);
  }
}

// (no second launch bound: asked for two waves per SIMD the 16-block instance spills 44 bytes per lane; left alone it
// takes 264 registers, 8 of them AGPRs, one wave per SIMD and no scratch - profiles/lev_long_dense.txt)
template <int NB>
__global__ __launch_bounds__(PG_WG_THREADS) void pg_levenshtein_long_dense_kernel(const LevLongParams p) {
  // per text position of the chunk: masks of planes 0..3 | plane 4; one spare entry for segment()'s look-ahead
  __shared__ uint4 amask[PG_WG_WAVES][PG_LEV_LONG_BLOCK + 1][2];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long ct = (long long)blockIdx.x % p.colTiles, rg = (long long)blockIdx.x / p.colTiles;
  const long long col = (ct * PG_WG_WAVES + wv) * 64 + lane;      // < colTiles * 256 <= xNpad
  const bool have = col < p.n;
  int lb = have ? p.xLens[col] : 0;
  lb = lb < 0 ? 0 : (lb > p.xl ? p.xl : lb);
  int mx = lb;                                                    // the longest pattern of the wave
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(mx, off);
    mx = o > mx ? o : mx;
  }
  const int nbw = __builtin_amdgcn_readfirstlane(blocks_of(mx));  // <= blocks_of(xl) <= NB
  const uint4 *am = &amask[wv][0][0] + opaque_zero();
  auto masks = [&](int j, u32 (&mk)[5]) {
    const uint4 m03 = am[j * 2];
    mk[0] = m03.x; mk[1] = m03.y; mk[2] = m03.z; mk[3] = m03.w;
    mk[4] = am[j * 2 + 1].x;
  };

  for (int r = 0; r < PG_LEVD_ROWS; ++r) {
    const long long row = rg * PG_LEVD_ROWS + r;
    if (row >= p.m) break;
    int la = __builtin_amdgcn_readfirstlane(p.yLens[row]);
    la = la < 0 ? 0 : (la > p.yl ? p.yl : la);
    u32 VP[NB][4], VN[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int w = 0; w < 4; ++w) { VP[b][w] = 0xFFFFFFFFu; VN[b][w] = 0u; }
    }
    for (int c0 = 0; c0 < la; c0 += PG_LEV_LONG_BLOCK) {          // la <= yl: chunk c0 / 128 is a block of the Y operand
      const int cnt = la - c0;                                    // text positions left, this chunk takes up to 128
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the previous chunk's reads are done
      __builtin_amdgcn_wave_barrier();
      for (int j = lane; j < PG_LEV_LONG_BLOCK; j += 64) {
        u32 mk[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
          const u32 *yw = (const u32 *)(p.yPlanes + ((long long)(c0 / PG_LEV_LONG_BLOCK) * 5 + q) * p.yNpad + row);
          mk[q] = 0u - ((yw[j >> 5] >> (j & 31)) & 1u);
        }
        amask[wv][j][0] = make_uint4(mk[0], mk[1], mk[2], mk[3]);
        amask[wv][j][1] = make_uint4(mk[4], 0u, 0u, 0u);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

      u32 hp[4] = {0u, 0u, 0u, 0u}, hn[4] = {0u, 0u, 0u, 0u};     // block b -> b + 1, 32 positions per pair
      lev_long_blocks<NB, 0>(p, (u32)col * 16u, nbw, cnt, masks, VP, VN, hp, hn);
    }
    int d = la;
#pragma unroll
    for (int b = 0; b < NB; ++b) d += pg_ll::readoff(VP[b], VN[b], lb, b);
    if (have) {
      if (p.outBytes == 2) ((_Float16 *)p.out)[row * p.ldo + col] = (_Float16)d;
      else ((long long *)p.out)[row * p.ldo + col] = (long long)d;
    }
  }
}

template <int NB>
static void lev_long_launch(const LevLongParams &p, long long blocks, hipStream_t s) {
  pg_levenshtein_long_dense_kernel<NB><<<dim3((unsigned)blocks), dim3(PG_WG_THREADS), 0, s>>>(p);
}

extern "C" {

int pg_lev_long_pack(const uint8_t *tokens, int64_t n, int l, int64_t ld, void *planes, int64_t npad, int32_t *lens,
                     uint32_t *flags, void *stream) {
  if (!tokens || !planes || !lens || !flags || n <= 0 || l <= 0 || ld < l) return pg_fail(PG_E_BADARG, "pg_lev_long_pack: bad argument");
  if (l > PG_LEV_LONG_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_lev_long_pack: at most 2048 positions");
  if (npad < n || npad % 256) return pg_fail(PG_E_BADARG, "pg_lev_long_pack: npad must be pg_npad(n)");
  hipStream_t s = (hipStream_t)stream;
  if (hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s)) return pg_launched((int)e, "pg_lev_long_pack");
  pg_lev_long_pack_kernel<<<dim3((unsigned)(npad / 256)), dim3(256), 0, s>>>(tokens, n, l, ld, (uint4 *)planes, npad, lens, flags);
  return pg_launched("pg_lev_long_pack_kernel");
}

int pg_levenshtein_long_dense(const void *x_planes, int64_t n, int64_t x_npad, const int32_t *x_lens, int xl,
                              const void *y_planes, int64_t m, int64_t y_npad, const int32_t *y_lens, int yl, void *out,
                              int out_elem_bytes, int64_t ldo, void *stream) {
  if (!x_planes || !x_lens || !y_planes || !y_lens || !out || n <= 0 || m <= 0 || xl <= 0 || yl <= 0 || ldo < n)
    return pg_fail(PG_E_BADARG, "pg_levenshtein_long_dense: bad argument");
  if (xl > PG_LEV_LONG_MAX_L || yl > PG_LEV_LONG_MAX_L)
    return pg_fail(PG_E_TOOLONG, "pg_levenshtein_long_dense: at most 2048 positions per operand");
  if (out_elem_bytes != 2 && out_elem_bytes != 8)
    return pg_fail(PG_E_BADARG, "pg_levenshtein_long_dense: out_elem_bytes must be 2 or 8");
  if (x_npad < n || x_npad % 256 || y_npad < m) return pg_fail(PG_E_BADARG, "pg_levenshtein_long_dense: bad npad");
  LevLongParams p;
  p.xPlanes = (const uint4 *)x_planes; p.xNpad = x_npad; p.n = n; p.xLens = x_lens; p.xl = xl;
  p.yPlanes = (const uint4 *)y_planes; p.yNpad = y_npad; p.m = m; p.yLens = y_lens; p.yl = yl;
  p.out = out; p.outBytes = out_elem_bytes; p.ldo = ldo;
  p.colTiles = (n + PG_WG_THREADS - 1) / PG_WG_THREADS;
  const long long blocks = p.colTiles * ((m + PG_LEVD_ROWS - 1) / PG_LEVD_ROWS);
  if (blocks > 0x7fffffffLL) return pg_fail(PG_E_TOOMANY, "pg_levenshtein_long_dense: too many blocks for one launch");
  hipStream_t s = (hipStream_t)stream;
  switch (pg_ll::instance_of(blocks_of(xl))) {                    // the pattern's blocks decide: they are the registers
    case 1: lev_long_launch<1>(p, blocks, s); break;
    case 2: lev_long_launch<2>(p, blocks, s); break;
    case 4: lev_long_launch<4>(p, blocks, s); break;
    case 8: lev_long_launch<8>(p, blocks, s); break;
    default: lev_long_launch<16>(p, blocks, s); break;
  }
  return pg_launched("pg_levenshtein_long_dense_kernel");
}

}  // extern "C"
