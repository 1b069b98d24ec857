// Probe of the CHAINED filter MFMA on gfx950 (pg_common.h, "chained filter MFMAs"): three column tiles accumulate
// into one result of v_mfma_scale_f32_32x32x64_f8f6f4 - block scales 2^-22 / 2^-14 / 2^-6 on the row operand, the
// chain starting from 2.0 - so that one test of (bits & PG_CHAIN_FLAGS) replaces three sign tests.
//   (a) the chain is bit exact against an integer reference: random operand sets in the engine's encoding (rows:
//       54 signature bits + ten bias nibbles from pg_bias_nibbles, columns as pg_pack_planes writes them, padding
//       columns all zero) and corner sets (every field at -114, -1, 0, 112 in all 64 combinations; bias -60 and 58);
//   (b) flag != 0  <=>  some field is negative, on those results;
//   (c) cycles per MFMA, one and three waves per SIMD: the in-place chain against independent unscaled MFMAs with
//       C = 0 (the loop before the chain), and the scaled against the unscaled form.
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-mfma-vgpr-form=1 mfma_fp4_chain.hip -o mfma_fp4_chain
#include "../../prograph_amd/csrc/pg_common.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// as in pg_mm.h: ONE scale register, the row operand takes byte `sel` of it, the column operand byte 3 (127: 1)
#define MFMA(a, b, c, sel, sa, sb) __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 4, sel, sa, 3, sb)

__host__ __device__ inline unsigned long long mix(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull; x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
constexpr unsigned long long kSigMask = (1ull << PG_SIG_BITS) - 1ull;

// ---- operand sets ----------------------------------------------------------------------------------------------
// engine encoding, wave w: row r has signature rsig and asks for bias rb; column c of tile t has signature csig, or is
// a padding column (all 64 elements zero).  Waves with (w & 15) == 0 hold the corners of the encoding.
struct Row { unsigned long long sig; int bias; };
struct Col { unsigned long long sig; bool pad; };
__device__ Row row_of(u32 w, int r) {
  const unsigned long long h = mix(((unsigned long long)w << 8) | (u32)r);
  if ((w & 15u) == 0u) return (r & 1) ? Row{0ull, 58} : Row{kSigMask, -60};
  const int kind = (int)((h >> 60) & 3);
  const int b = kind == 0 ? -60 : (kind == 1 ? (int)((h >> 40) % 141u) - 70 : (int)((h >> 40) % 13u) - 6);   // open bounds, any, near zero
  return Row{h & kSigMask, b};
}
__device__ Col col_of(u32 w, int t, int c) {
  const unsigned long long h = mix(0x5000000000ull | ((unsigned long long)w << 12) | ((u32)t << 8) | (u32)c);
  if ((w & 15u) == 0u) return c % 3 == 0 ? Col{kSigMask, false} : (c % 3 == 1 ? Col{0ull, false} : Col{0ull, true});
  const int kind = (int)((h >> 60) & 7);
  if (kind == 0) return Col{0ull, true};
  if (kind == 1) return Col{h & kSigMask, false};                                   // unrelated
  unsigned long long s = row_of(w, (c + t) & 31).sig;                               // a neighbour of some row: up to 12 bits away
  const int flips = (int)((h >> 54) % 13u);
  for (int i = 0; i < flips; ++i) s ^= 1ull << (mix(h + i) % PG_SIG_BITS);
  return Col{s, false};
}
__device__ int dval(const Row &r, const Col &c) {
  if (c.pad) return 0;
  return __popcll(r.sig ^ c.sig) - __popcll(r.sig) + pg_bias_nibbles_sum2(pg_bias_nibbles(r.bias)) / 2;
}

// counters: 0 sets, 1 value mismatches, 2 flag mismatches, 3 sets with a negative field, 4 of them with S >= 0,
// 5 mismatches against pg_chain_value, 6 / 7 = -min / max field seen (+0)
__device__ void check(const v16f &x, int lane, const int (&d)[16][3], unsigned long long *cnt) {
  unsigned long long n = 0, bv = 0, bf = 0, ng = 0, ngp = 0, bh = 0;
  int lo = 0, hi = 0;
  for (int r = 0; r < 16; ++r) {
    const int S = d[r][0] + 256 * d[r][1] + 65536 * d[r][2];
    const float ref = (float)((1 << 23) + S) * 0x1p-22f;                              // an integer below 2^24: exact
    const u32 xb = __float_as_uint(x[r]);
    const bool anyneg = d[r][0] < 0 || d[r][1] < 0 || d[r][2] < 0;
    ++n;
    bv += xb != __float_as_uint(ref);
    bh += xb != __float_as_uint(pg_chain_value(d[r][0], d[r][1], d[r][2]));
    bf += (pg_chain_flag(xb) != 0u) != anyneg;
    ng += anyneg;
    ngp += anyneg && S >= 0;
    for (int t = 0; t < 3; ++t) { lo = d[r][t] < lo ? d[r][t] : lo; hi = d[r][t] > hi ? d[r][t] : hi; }
  }
  atomicAdd(&cnt[0], n); atomicAdd(&cnt[1], bv); atomicAdd(&cnt[2], bf); atomicAdd(&cnt[3], ng); atomicAdd(&cnt[4], ngp); atomicAdd(&cnt[5], bh);
  atomicMax(&cnt[6], (unsigned long long)-lo); atomicMax(&cnt[7], (unsigned long long)hi);
}

// the chains as pg_mm.h issues them (the inline-assembly statements of pg_common.h): LEN 3 = first result of
// pg_chain_3x2, 4 = its second (the operands given twice), 2 = pg_chain_2 + pg_chain_settle, 1 = second result of pg_chain_3p1
template <int LEN> __device__ v16f chain(const v8i &A8, const v8i (&B8)[3]) {
  const int sc = (int)opaque_vgpr(PG_CHAIN_SCALE_A);
  const pg_v4i A = {A8[0], A8[1], A8[2], A8[3]};
  pg_v4i B[3];
  for (int t = 0; t < 3; ++t) B[t] = pg_v4i{B8[t][0], B8[t][1], B8[t][2], B8[t][3]};
  pg_v16f x, y;
  if (LEN >= 3) {
    pg_chain_3x2(x, y, A, A, B[0], B[1], B[2], sc);
    return LEN == 3 ? x : y;
  }
  if (LEN == 2) {
    pg_chain_3x2(y, x, A, A, B[2], B[1], B[0], sc);           // (something in the pipe in front, as in the loop)
    pg_chain_2(x, y, A, B[0], A, B[1], sc);
    pg_chain_settle(x);
    return x;
  }
  pg_chain_3p1(x, y, A, B[2], B[1], B[1], B[0], sc);
  return y;
}

// one wave per operand set group: 32 rows x 32 columns x 3 tiles = 1024 sets
template <int LEN> __global__ void verify_engine(u32 w0, unsigned long long *cnt) {
  constexpr int NT = LEN > 3 ? 3 : LEN;
  const int lane = threadIdx.x & 63;
  const u32 w = w0 + blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const Row me = row_of(w, lane & 31);
  const u32 half = lane >> 5 ? (u32)(me.sig >> 32) : (u32)me.sig;
  v8i A = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) A[i] = (int)(0x22222222u | (pg_nib8(half >> (8 * i)) << 3));
  if (lane >= 32) {                                                                  // pg_mm.h, encode_bias
    const unsigned long long nb = pg_bias_nibbles(me.bias);
    A[2] = (int)(((u32)A[2] & 0x00FFFFFFu) | ((u32)nb << 24));
    A[3] = (int)(u32)(nb >> 8);
  }
  v8i B[3];
  for (int t = 0; t < 3; ++t) {
    const Col c = col_of(w, t, lane & 31);
    const u32 lo = (u32)c.sig, hi = (u32)(c.sig >> 32) | (c.pad ? 0u : 0xFFC00000u);   // pg_api.hip, pg_pack_planes
    const u32 x = lane >> 5 ? hi : lo;
    B[t] = v8i{(int)(pg_nib8(x) << 1), (int)(pg_nib8(x >> 8) << 1), (int)(pg_nib8(x >> 16) << 1), (int)(pg_nib8(x >> 24) << 1), 0, 0, 0, 0};
  }
  const v16f x = chain<LEN>(A, B);
  int d[16][3];
  for (int r = 0; r < 16; ++r) {
    const Row rr = row_of(w, (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5));
    for (int t = 0; t < 3; ++t) d[r][t] = t < NT ? dval(rr, col_of(w, t, lane & 31)) : 0;
  }
  check(x, lane, d, cnt);
}

// corner sets outside the encoding's reach for ONE row: every row holds -6 x 19 | +6 x 18, +4 | -1 | 0 .., a column
// selects one group (B = 1 there): fields -114, 112, -1, 0.  Column cc = c + 32 * wave takes type (cc >> 2t) & 3 in
// tile t: two waves cover all 64 combinations, in every row.
__global__ void verify_corners(unsigned long long *cnt) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  constexpr int val[4] = {-114, 112, -1, 0};
  v8i A = {0, 0, 0, 0, 0, 0, 0, 0};
  v8i B[3];
  for (int t = 0; t < 3; ++t) B[t] = v8i{0, 0, 0, 0, 0, 0, 0, 0};
  int ty[3];
  for (int t = 0; t < 3; ++t) ty[t] = (((lane & 31) + 32 * wv) >> (2 * t)) & 3;
  for (int j = 0; j < 32; ++j) {
    const int k = 32 * (lane >> 5) + j;
    const u32 a = k < 19 ? 0xFu : (k < 37 ? 0x7u : (k == 37 ? 0x6u : (k == 38 ? 0xAu : 0x0u)));
    const int grp = k < 19 ? 0 : (k < 38 ? 1 : (k == 38 ? 2 : 3));
    A[j / 8] |= (int)(a << (4 * (j % 8)));
    for (int t = 0; t < 3; ++t) B[t][j / 8] |= (grp == ty[t] && grp != 3) ? (int)(0x2u << (4 * (j % 8))) : 0;
  }
  const v16f x = chain<3>(A, B);
  int d[16][3];
  for (int r = 0; r < 16; ++r)
    for (int t = 0; t < 3; ++t) d[r][t] = val[ty[t]];
  check(x, lane, d, cnt);
}

// ---- (c) issue rate ---------------------------------------------------------------------------------------------
// MODE 0: independent unscaled MFMAs, C = 0, two result sets in turn (the loop before the chain)
//      1: independent SCALED MFMAs, C = 2.0 (every one a chain head), two result sets in turn
//      2: one in-place chain: head + 2 accumulating, again and again on the same registers
//      3: two chains interleaved (head, head, acc, acc, acc, acc)
//      4: unscaled in-place accumulation on one register set
//      5: the statements of the R = 2 loop: pg_chain_3x2, pg_chain_2, pg_chain_settle (8 MFMAs and 26 wait states of s_nop)
template <int MODE> __global__ void rate(int iters, const u32 *src, unsigned long long *cyc, float *sink) {
  const int lane = threadIdx.x & 63;
  v8i A = {0, 0, 0, 0, 0, 0, 0, 0}, B = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) { A[i] = (int)src[lane * 4 + i]; B[i] = (int)src[256 + lane * 4 + i]; }
  const int sa = (int)PG_CHAIN_SCALE_A, sb = sa;
  v16f x = {0}, y = {0}, two, zero = {0};
  for (int r = 0; r < 16; ++r) two[r] = PG_CHAIN_BASE;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int i = 0; i < iters; ++i) {
    if (MODE == 0) {
      x = MFMA(A, B, zero, 0, 0, 0); y = MFMA(A, B, zero, 0, 0, 0); asm volatile("" : "+v"(x), "+v"(y));
      x = MFMA(A, B, zero, 0, 0, 0); y = MFMA(A, B, zero, 0, 0, 0); asm volatile("" : "+v"(x), "+v"(y));
      x = MFMA(A, B, zero, 0, 0, 0); y = MFMA(A, B, zero, 0, 0, 0); asm volatile("" : "+v"(x), "+v"(y));
    } else if (MODE == 1) {
      x = MFMA(A, B, two, 0, sa, sb); y = MFMA(A, B, two, 1, sa, sb); asm volatile("" : "+v"(x), "+v"(y));
      x = MFMA(A, B, two, 2, sa, sb); y = MFMA(A, B, two, 0, sa, sb); asm volatile("" : "+v"(x), "+v"(y));
      x = MFMA(A, B, two, 1, sa, sb); y = MFMA(A, B, two, 2, sa, sb); asm volatile("" : "+v"(x), "+v"(y));
    } else if (MODE == 2) {
      x = MFMA(A, B, two, 0, sa, sb); x = MFMA(A, B, x, 1, sa, sb); x = MFMA(A, B, x, 2, sa, sb); asm volatile("" : "+v"(x));
      x = MFMA(A, B, two, 0, sa, sb); x = MFMA(A, B, x, 1, sa, sb); x = MFMA(A, B, x, 2, sa, sb); asm volatile("" : "+v"(x));
    } else if (MODE == 3) {
      x = MFMA(A, B, two, 0, sa, sb); y = MFMA(A, B, two, 0, sa, sb);
      x = MFMA(A, B, x, 1, sa, sb); y = MFMA(A, B, y, 1, sa, sb);
      x = MFMA(A, B, x, 2, sa, sb); y = MFMA(A, B, y, 2, sa, sb); asm volatile("" : "+v"(x), "+v"(y));
    } else if (MODE == 5) {
      const pg_v4i a = {A[0], A[1], A[2], A[3]}, b = {B[0], B[1], B[2], B[3]};
      pg_v16f z;
      pg_chain_3x2(x, y, a, a, b, b, b, sa); pg_chain_2(z, y, a, b, a, b, sa); pg_chain_settle(z);
      asm volatile("" : "+v"(x), "+v"(y), "+v"(z));
    } else {
      x = MFMA(A, B, zero, 0, 0, 0); x = MFMA(A, B, x, 0, 0, 0); x = MFMA(A, B, x, 0, 0, 0); asm volatile("" : "+v"(x));
      x = MFMA(A, B, zero, 0, 0, 0); x = MFMA(A, B, x, 0, 0, 0); x = MFMA(A, B, x, 0, 0, 0); asm volatile("" : "+v"(x));
    }
  }
  asm volatile("s_nop 15\n\ts_nop 15" : "+v"(x), "+v"(y));
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) cyc[blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)] = t1 - t0;
  if (iters < 0) sink[threadIdx.x] = x[0] + y[0];
}

#define CK(e) do { hipError_t err_ = (e); if (err_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(err_), __LINE__); return 2; } } while (0)

template <int MODE> static int run_rate(const char *what, const u32 *dsrc, unsigned long long *dcyc, float *dsink) {
  const int iters = 20000, blocks = 64;
  for (int wps = 1; wps <= 3; wps += 2) {
    const int nw = blocks * 4 * wps;
    rate<MODE><<<blocks, 256 * wps>>>(iters, dsrc, dcyc, dsink);
    rate<MODE><<<blocks, 256 * wps>>>(iters, dsrc, dcyc, dsink);
    CK(hipDeviceSynchronize());
    std::vector<unsigned long long> c(nw);
    CK(hipMemcpy(c.data(), dcyc, nw * 8, hipMemcpyDeviceToHost));
    double s = 0;
    for (auto v : c) s += (double)v;
    const double perWave = s / nw / ((double)iters * (MODE == 5 ? 8 : 6));
    printf("  %-58s %d wave(s)/SIMD: %6.1f cycles per MFMA and wave, %5.1f per MFMA and SIMD\n", what, wps, perWave, perWave / wps);
  }
  return 0;
}

int main() {
  unsigned long long *dcnt;
  CK(hipMalloc(&dcnt, 8 * 8));
  unsigned long long h[8];
  int fail = 0;
  auto report = [&](const char *what) {
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, dcnt, 64, hipMemcpyDeviceToHost) != hipSuccess) { printf("HIP error in %s\n", what); fail = 2; return; }
    printf("%-34s %9llu sets: %llu value mismatches (integer reference), %llu against pg_chain_value, %llu flag mismatches; "
           "%llu sets with a negative field, %llu of them with S >= 0; fields in [-%llu, %llu]\n",
           what, h[0], h[1], h[5], h[2], h[3], h[4], h[6], h[7]);
    if (h[1] || h[2] || h[5] || !h[0]) fail = 1;
  };
  printf("(a) + (b): chained v_mfma_scale_f32_32x32x64_f8f6f4, FP4, base 2.0, row scales 2^-22 / 2^-14 / 2^-6, flags 0x%08X\n", PG_CHAIN_FLAGS);
  const int waves = 1536;                                                            // x 1024 sets
  CK(hipMemset(dcnt, 0, 64)); verify_engine<3><<<waves / 4, 256>>>(0u, dcnt); report("engine encoding, chain of 3");
  CK(hipMemset(dcnt, 0, 64)); verify_engine<4><<<waves / 4, 256>>>(50000u, dcnt); report("engine encoding, chain of 3 (2nd)");
  CK(hipMemset(dcnt, 0, 64)); verify_engine<2><<<waves / 4, 256>>>(100000u, dcnt); report("engine encoding, chain of 2");
  CK(hipMemset(dcnt, 0, 64)); verify_engine<1><<<waves / 4, 256>>>(200000u, dcnt); report("engine encoding, chain of 1");
  CK(hipMemset(dcnt, 0, 64)); verify_corners<<<1, 128>>>(dcnt); report("corners {-114, 112, -1, 0}^3");
  printf("%s\n", fail ? "CHAIN NOT EXACT" : "chain exact, flag identity holds");
  if (fail) return fail;

  printf("(c) issue rate, 64 workgroups, 120000 (the R = 2 step: 160000) MFMAs per wave, cycles of s_memtime\n");
  std::vector<u32> src(512);
  for (int i = 0; i < 512; ++i) src[i] = i < 256 ? 0x22222222u | ((u32)mix(i) & 0x88888888u) : (u32)mix(i) & 0x22222222u;
  u32 *dsrc; unsigned long long *dcyc; float *dsink;
  CK(hipMalloc(&dsrc, 2048)); CK(hipMalloc(&dcyc, 64 * 12 * 8)); CK(hipMalloc(&dsink, 768 * 4));
  CK(hipMemcpy(dsrc, src.data(), 2048, hipMemcpyHostToDevice));
  if (run_rate<0>("independent, unscaled, C = 0 (the loop before)", dsrc, dcyc, dsink)) return 2;
  if (run_rate<1>("independent, scaled, C = 2.0", dsrc, dcyc, dsink)) return 2;
  if (run_rate<2>("one chain in place: head + 2, scaled", dsrc, dcyc, dsink)) return 2;
  if (run_rate<3>("two chains interleaved, scaled", dsrc, dcyc, dsink)) return 2;
  if (run_rate<5>("the R = 2 step: 3 + 3 + 2 with their s_nops", dsrc, dcyc, dsink)) return 2;
  if (run_rate<4>("one chain in place: head + 2, unscaled", dsrc, dcyc, dsink)) return 2;
  return 0;
}
