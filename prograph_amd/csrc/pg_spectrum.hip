// k-mer spectrum profiles - BUILD DEFINED: the count vector of every row of a uint8 token matrix, as
// the fp16 (n, D) matrix the cosine and Euclidean engines of pg_cos.hip take as it is.  Which windows count and the
// bucket of each is pg_spectrum.h, the same lines the CPU checker compiles.
//
// Kernel (pg_spectrum_kernel<HD, W>): one wave per sequence, W waves per workgroup, a bounded grid striding over the
// rows.  A wave stages its row in LDS (dwords when the row is 4-byte aligned) and learns its length - the position after
// the last non-zero token - on the way, so trailing padding costs no window; tokens above `symbols` raise the flag word
// with a plain store (every writer stores the same 1).  The histogram sits in LDS as HD dwords of two 16-bit counts, zeroed
// 16 bytes per lane; lanes stride over the windows, read their k tokens from LDS and add 1 << 16 (bucket & 1) to dword
// bucket >> 1 with a 32-bit LDS atomic - a count is at most 2048, so it never carries into its neighbour.  The write-out
// turns four dwords into eight fp16 and stores 16 bytes per lane, coalesced along the row; a row whose start is not 16-byte
// aligned (an odd ldo) and the last D mod 8 elements go out as 2-byte stores.  Exactly D elements per row are written.
// No global atomics, no scratch, no workspace.
//
// Instances by histogram size, all static LDS: D <= 1024 -> <512, 4> (16 KiB per workgroup), D <= 8192 -> <4096, 4>
// (72 KiB: two workgroups per CU), else <16384, 2> (132 KiB: one).
#include "pg_common.h"
#include "pg_spectrum.h"
#include "../../include/prograph_hip.h"

struct SpectrumParams {
  const unsigned char *tok;
  long long n, ld;
  int l;
  const long long *rows;      // optional gather list: output row r is token row rows[r]
  int k, symbols, shift, D;
  _Float16 *out;
  long long ldo;
  u32 *flags;
};

typedef _Float16 pg_sp_h2 __attribute__((ext_vector_type(2)));

// the lanes of a wave have finished their LDS accesses before any of them goes on
__device__ __forceinline__ void sp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// two 16-bit counts -> two fp16 in the same halves
__device__ __forceinline__ u32 sp_pair_f16(u32 c) {
  pg_sp_h2 h;
  h.x = (_Float16)(unsigned short)(c & 0xffffu);
  h.y = (_Float16)(unsigned short)(c >> 16);
  return __builtin_bit_cast(u32, h);
}

template <int HD, int W>
__global__ __launch_bounds__(PG_WAVE * W) void pg_spectrum_kernel(const SpectrumParams p) {
  __shared__ __attribute__((aligned(16))) u32 hist[W][HD];
  __shared__ __attribute__((aligned(16))) unsigned char toks[W][PG_SP_MAX_L + 16];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  u32 *const h = hist[wv];
  unsigned char *const tw = toks[wv];
  const int hd = (p.D + 1) >> 1;                    // dwords in use (<= HD: the launcher's choice of instance)
  const int hd4 = (hd + 3) & ~3;                    // (HD is a multiple of 4)
  u32 bad = 0u;

  for (long long r = (long long)blockIdx.x * W + wv; r < p.n; r += (long long)gridDim.x * W) {
    const unsigned char *row = p.tok + (p.rows ? p.rows[r] : r) * p.ld;
    // ---- stage the row, find its length, check its tokens
    int len = 0;
    if ((((uintptr_t)row) & 3u) == 0) {
      const int nd = p.l >> 2;
      for (int i = lane; i < nd; i += 64) {
        const u32 w = ((const u32 *)row)[i];
        ((u32 *)tw)[i] = w;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const u32 t = (w >> (8 * b)) & 255u;
          if (t > (u32)p.symbols) bad = 1u;
          if (t) len = 4 * i + b + 1;
        }
      }
      for (int i = 4 * nd + lane; i < p.l; i += 64) {
        const u32 t = row[i];
        tw[i] = (unsigned char)t;
        if (t > (u32)p.symbols) bad = 1u;
        if (t) len = i + 1;
      }
    } else {
      for (int i = lane; i < p.l; i += 64) {
        const u32 t = row[i];
        tw[i] = (unsigned char)t;
        if (t > (u32)p.symbols) bad = 1u;
        if (t) len = i + 1;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int o = __shfl_xor(len, off);
      len = o > len ? o : len;
    }
    len = __builtin_amdgcn_readfirstlane(len);      // <= l
    // ---- zero the histogram
    for (int i = 4 * lane; i < hd4; i += 256) *(uint4 *)(h + i) = make_uint4(0u, 0u, 0u, 0u);
    sp_wave_sync();
    // ---- the windows
    const int nwin = len - p.k + 1;                 // windows past the last non-zero token hold a 0
    for (int i = lane; i < nwin; i += 64) {
      uint32_t bucket;
      if (pg_sp_window(tw + i, p.k, p.symbols, p.shift, &bucket) && bucket < (u32)p.D)
        atomicAdd(h + (bucket >> 1), 1u << (16 * (bucket & 1u)));
    }
    sp_wave_sync();
    // ---- write the row out
    _Float16 *orow = p.out + r * p.ldo;
    int done = 0;
    if ((((uintptr_t)orow) & 15u) == 0) {
      const int ng = p.D >> 3;
      for (int j = lane; j < ng; j += 64) {
        const uint4 c = *(const uint4 *)(h + 4 * j);
        *(uint4 *)(orow + 8 * j) = make_uint4(sp_pair_f16(c.x), sp_pair_f16(c.y), sp_pair_f16(c.z), sp_pair_f16(c.w));
      }
      done = ng << 3;
    }
    for (int e = done + lane; e < p.D; e += 64) orow[e] = (_Float16)(unsigned short)((h[e >> 1] >> (16 * (e & 1))) & 0xffffu);
    sp_wave_sync();                                 // the reads are done before the next row zeroes
  }
  if (__any((int)bad) && lane == 0) *p.flags = 1u;
}

template <int HD, int W>
static void spectrum_launch(const SpectrumParams &p, hipStream_t s) {
  long long blocks = (p.n + W - 1) / W;
  if (blocks > 2048) blocks = 2048;                 // the grid strides over the rows
  pg_spectrum_kernel<HD, W><<<dim3((unsigned)blocks), dim3(PG_WAVE * W), 0, s>>>(p);
}

extern "C" {

int pg_spectrum_dims(int k, int symbols, int dims) {
  const int D = pg_sp_dims(k, symbols, dims);
  if (D < 0)
    return pg_fail(PG_E_BADARG, "pg_spectrum_dims: k in 1..6, symbols in 2..255, symbols^k <= 2^31 (<= 32768 with dims 0), dims 0 or "
                                "a power of two in 64..32768");
  return D;
}

int pg_spectrum_profile(const uint8_t *tokens, int64_t n, int l, int64_t ld, const int64_t *rows, int k, int symbols, int dims,
                        void *out_f16, int64_t ldo, int32_t *flags, void *stream) {
  const int D = pg_spectrum_dims(k, symbols, dims);
  if (D < 0) return D;
  if (!tokens || !out_f16 || !flags || n <= 0 || l <= 0 || ld < l || ldo < D) return pg_fail(PG_E_BADARG, "pg_spectrum_profile: bad argument");
  if (l > PG_SP_MAX_L) return pg_fail(PG_E_TOOLONG, "pg_spectrum_profile: at most 2048 positions");
  SpectrumParams p;
  p.tok = tokens; p.n = n; p.ld = ld; p.l = l; p.rows = (const long long *)rows;
  p.k = k; p.symbols = symbols; p.shift = pg_sp_shift(dims); p.D = D;
  p.out = (_Float16 *)out_f16; p.ldo = ldo; p.flags = (u32 *)flags;
  hipStream_t s = (hipStream_t)stream;
  if (hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s)) return pg_launched((int)e, "pg_spectrum_profile");
  if (D <= 1024) spectrum_launch<512, 4>(p, s);
  else if (D <= 8192) spectrum_launch<4096, 4>(p, s);
  else spectrum_launch<16384, 2>(p, s);
  return pg_launched("pg_spectrum_kernel");
}

}  // extern "C"
