// C ABI of the hot path (include/prograph_hip.h) + the O(N*L) helper kernels:
// plane packing, exclusive scan, flag compaction and the fused 1xN indexing pass.
#include "pg_common.h"
#include "pg_mm.h"
#include "pg_plan.h"   // host-only: the planners, the workspace layout, the knobs
#include "../../include/prograph_hip.h"

#include <dlfcn.h>
#include <math.h>
#include <rccl/rccl.h>   // types only: the library is resolved at run time (dlopen), there is no link dependency
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>

static thread_local char g_err[256] = "";

void pg_set_error(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }

// the PG_* knobs of a C-ABI call (table and reader: pg_plan.h), read from the environment once per call
extern char **environ;
static PgKnobs read_knobs() { return pg_knobs_read(environ); }

// compute units of the CURRENT device (cached per device: a process may drive several)
#define PG_MAX_DEVICES 64
static int cu_count() {
  static std::atomic<int> cus[PG_MAX_DEVICES];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  const bool cached = dev >= 0 && dev < PG_MAX_DEVICES;
  if (cached && cus[dev].load(std::memory_order_relaxed) > 0) return cus[dev].load(std::memory_order_relaxed);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
  if (cached) cus[dev].store(prop.multiProcessorCount, std::memory_order_relaxed);
  return prop.multiProcessorCount;
}

extern "C" {

int pg_version(void) { return PG_ABI_VERSION; }
const char *pg_last_error(void) { return g_err; }

int pg_device_info(int *cus, int *wave, char *arch, int arch_len) {
  int dev = 0;
  hipDeviceProp_t prop;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return pg_launched((int)e, "hipGetDevice");
  e = hipGetDeviceProperties(&prop, dev);
  if (e != hipSuccess) return pg_launched((int)e, "hipGetDeviceProperties");
  if (cus) *cus = prop.multiProcessorCount;
  if (wave) *wave = prop.warpSize;
  if (arch && arch_len > 0) snprintf(arch, (size_t)arch_len, "%s", prop.gcnArchName);
  return 0;
}

int64_t pg_npad(int64_t n) { return n <= 0 ? 256 : ((n + 255) / 256) * 256; }
int pg_ngroups(int l) { return plan_ngroups(l); }
int pg_nchunks(int l, int bits) { return plan_nchunks(l, bits); }
int64_t pg_planes_bytes(int64_t n, int l, int bits) { return ((int64_t)pg_nchunks(l, bits) * 16 + PG_AUX_BYTES) * pg_npad(n); }
// launch-private device state of an all-pairs call, sized by the row count (the layout: pg_plan.h)
int64_t pg_workspace_bytes(int64_t nrows) { return workspace_bytes(nrows, cu_count(), read_knobs()); }

}  // extern "C"

// The plan of the symmetric kNN sweep on the device (sym_block_pieces, sym_piece_range: pg_plan.h - the same code as the host's).
// workgroup 0: thread t takes a contiguous run of blocks - their piece counts, a scan over the threads, then the
// entries and pieceStart[b] = the first pass of block b (pieceStart[nb] = passes in all).  The workgroups behind it zero
// the rows' counts of delivered keys meanwhile (`zero4` uint4 of lowCount: the launch's memset, folded in)
// The scan: a thread of up to four blocks (up to 262 144 rows) keeps their counts in a register - one sym_block_pieces, with its
// 64-bit division, a block - and recomputes them beyond; an inclusive scan inside every wave (six shuffles), the sixteen
// waves' totals through LDS behind ONE barrier, every thread adds up the totals of the waves in front of it.
// The function is the whole workgroup's (1024 threads, a barrier in it): workgroup `vb` of `vgrid`.  pg_knn_sym_plan_kernel
// is a launch of its own - symmetric launches without a probe -, behind a probe its workgroups ride in pg_decide_kernel's
// launch (KnnPlan::symPlanRides): the plan needs the shape and the workspace alone, and the sweep waits for neither twice.
struct SymPlanArgs {
  long long nb, nst, slots;
  int piece, pmin;
  int4 *plan;
  u32 *pieceStart;
  uint4 *zero;
  long long zero4;
  unsigned grid;             // workgroups: one plans, the rest zero (0: nothing rides)
};
static __device__ __forceinline__ void sym_plan_workgroup(unsigned vb, unsigned vgrid, const SymPlanArgs &a) {
  __shared__ u32 waveTotal[16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (vb > 0) {
    for (long long i = (long long)(vb - 1) * 1024 + t; i < a.zero4; i += (long long)(vgrid - 1) * 1024) a.zero[i] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const long long nb = a.nb, per = (nb + 1023) / 1024, b0 = t * per, b1 = b0 + per < nb ? b0 + per : nb;
  const bool few = per <= 4;
  u32 np4 = 0u, mine = 0;                                  // (four counts of at most 16, a byte each; one copy of the division: no unrolling)
  if (few) {
#pragma unroll 1
    for (int j = 0; b0 + j < b1; ++j) {
      const u32 np = (u32)sym_block_pieces(b0 + j, a.nst, a.slots, a.piece, a.pmin);
      np4 |= np << (8 * j);
      mine += np;
    }
  } else {
    // (one copy here too: the loop vectoriser makes sixteen of the division, which spill)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (long long b = b0; b < b1; ++b) mine += (u32)sym_block_pieces(b, a.nst, a.slots, a.piece, a.pmin);
  }
  u32 incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 x = (u32)__shfl_up((int)incl, o);
    incl += lane >= o ? x : 0u;
  }
  if (lane == 63) waveTotal[wv] = incl;
  __syncthreads();
  u32 front = 0, total = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const u32 x = waveTotal[i];
    front += i < wv ? x : 0u;
    total += x;
  }
  u32 at = front + incl - mine;
  auto entries = [&](long long b, int np) {
    a.pieceStart[b] = at;
#pragma unroll 1
    for (int q = 0; q < np; ++q, ++at) {                     // (one copy of the loop body: unrolled it spills, and the decision launch would need scratch)
      int f, e;
      sym_piece_range(b, a.nst, np, q, &f, &e);
      a.plan[at] = make_int4((int)b, f, e, q);
    }
  };
  if (few) {
#pragma unroll 1
    for (int j = 0; b0 + j < b1; ++j) entries(b0 + j, (int)((np4 >> (8 * j)) & 0xFFu));
  } else {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (long long b = b0; b < b1; ++b) entries(b, sym_block_pieces(b, a.nst, a.slots, a.piece, a.pmin));
  }
  if (t == 1023) a.pieceStart[nb] = total;
}
__global__ __launch_bounds__(1024) void pg_knn_sym_plan_kernel(SymPlanArgs a) { sym_plan_workgroup(blockIdx.x, gridDim.x, a); }
extern "C" {
// the plan of the symmetric kNN sweep of an n x n self graph for `slots` waves (host only, no device needed): up to
// max_passes entries (row block, first super-tile, end super-tile, piece of the block) to out[4 * i ..]; returns the
// number of passes.  piece > 0: fixed piece length; piece_min: the guided rule's shortest piece (0: the default)
int64_t pg_knn_sym_plan(int64_t n, int64_t slots, int piece, int piece_min, int32_t *out, int64_t max_passes) {
  if (n <= 0 || slots <= 0) return pg_fail(PG_E_BADARG, "pg_knn_sym_plan: bad argument");
  return sym_plan_host(n, slots, piece, piece_min > 0 ? piece_min : (int)read_knobs().symPieceMin.v, out, max_passes);
}
// the same plan as pg_knn_sym_plan_kernel writes it (tests: the device plan against the host's without a kNN launch):
// plan_out: device memory for max_passes entries of four ints, piece_start_out: (n + 63) / 64 + 1 words; returns the number
// of passes, an error where they exceed max_passes (nothing is launched then)
int64_t pg_knn_sym_plan_device(int64_t n, int64_t slots, int piece, int piece_min, int32_t *plan_out, uint32_t *piece_start_out,
                               int64_t max_passes, void *stream) {
  if (n <= 0 || n > PG_MAX_N_KNN || slots <= 0 || !plan_out || !piece_start_out) return pg_fail(PG_E_BADARG, "pg_knn_sym_plan_device: bad argument");
  const int pmin = piece_min > 0 ? piece_min : (int)read_knobs().symPieceMin.v;
  const int64_t passes = sym_plan_host(n, slots, piece, pmin, nullptr, 0);
  if (passes > max_passes) return pg_fail(PG_E_BADARG, "pg_knn_sym_plan_device: the plan has more passes than max_passes");
  SymPlanArgs a = {(n + 63) / 64, (n + PG_MM_ST - 1) / PG_MM_ST, slots, piece, pmin, (int4 *)plan_out, piece_start_out, nullptr, 0, 1u};
  pg_knn_sym_plan_kernel<<<dim3(1), dim3(1024), 0, (hipStream_t)stream>>>(a);
  if (int rc = pg_launched("pg_knn_sym_plan_kernel")) return rc;
  return passes;
}
}  // extern "C"

// =======================================================================================
// pack: row-major tokens -> bit-sliced records in chunk-major order
// =======================================================================================
// A workgroup packs PG_PACK_SEQS consecutive sequences.  Work item (sequence, group): one lane gathers the 32 tokens of a
// group as 32 bytes - 16-byte loads where the base, the row stride and the group allow, position by position otherwise -
// and bit-slices them with four 8 x 8 bit transposes (word-level: no shift-and-or per bit and plane).  Items are
// sequence-major, so the lanes of a wave read a contiguous stretch of a dense token matrix.  The plane words meet in
// LDS in record order; one lane per (chunk, sequence) then stores a whole uint4 - a wave writes 1 KiB of a chunk array
// - and the signature and fold sections are made from the LDS copy.
// lut / tokOut (pg_pack_bytes): src holds the fixed-width BYTES of the sequences; token = lut[byte]
// (the reference's letter table, prograph/prograph.py:127,454-474: unknown bytes and padding -> 0), written row-major
// to tokOut as well when that is not NULL.
#define PG_PACK_SEQS 64
#define PG_PACK_LD 68        // LDS words per sequence: up to 8 groups x 8 planes, padded (16-byte aligned rows)

// 8 x 8 bit transpose: byte i bit p of x -> byte p bit i (Hacker's Delight 7-3, three swap stages)
__host__ __device__ __forceinline__ unsigned long long pg_transpose8(unsigned long long x) {
  unsigned long long t;
  t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;  x = x ^ t ^ (t << 7);
  t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x = x ^ t ^ (t << 14);
  t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x = x ^ t ^ (t << 28);
  return x;
}

template <typename T, int B>
__global__ __launch_bounds__(256) void pg_pack_kernel(const T *__restrict__ src, long long n, int l, long long ld,
                                                      const long long *__restrict__ rows, u32 *__restrict__ planes,
                                                      long long npad, int ng, int nq, u32 *flags,
                                                      const unsigned char *__restrict__ lut = nullptr,
                                                      unsigned char *__restrict__ tokOut = nullptr) {
  constexpr int E = (int)sizeof(T), PER = 16 / E;           // tokens per 16-byte load
  __shared__ __attribute__((aligned(16))) u32 words[PG_PACK_SEQS * PG_PACK_LD];
  const long long s0 = (long long)blockIdx.x * PG_PACK_SEQS;   // (npad is a multiple of 256: whole workgroups)
  const int tid = threadIdx.x;
  // 16-byte loads: every row and every group of 32 tokens starts on a 16-byte boundary
  const bool vec = !lut && ((unsigned long long)src & 15ull) == 0 && ((ld * E) & 15ll) == 0;
  for (int item = tid; item < PG_PACK_SEQS * ng; item += 256) {
    const int sl = item / ng, g = item - sl * ng;
    const long long s = s0 + sl;
    unsigned long long x[4] = {0, 0, 0, 0}, high = 0;     // the group's tokens, one byte each; OR of all bits of the elements
    if (s < n) {
      const T *row = src + (rows ? rows[s] : s) * ld;
      if (vec && g * 32 + 32 <= l) {
        const uint4 *r16 = reinterpret_cast<const uint4 *>(row + g * 32);
#pragma unroll
        for (int c = 0; c < 32 / PER; ++c) {
          const uint4 v = r16[c];
          T e[PER];
          __builtin_memcpy(e, &v, 16);
#pragma unroll
          for (int i = 0; i < PER; ++i) {
            const int j = c * PER + i;
            const unsigned long long t = (unsigned long long)(long long)e[i];
            high |= t;
            x[j >> 3] |= (t & 0xFFull) << (8 * (j & 7));
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 32; ++j) {
          const int pos = g * 32 + j;
          if (pos < l) {
            long long v = (long long)row[pos];
            if (lut) {
              v = lut[(unsigned char)v];
              if (tokOut) tokOut[s * (long long)l + pos] = (unsigned char)v;
            }
            high |= (unsigned long long)v;
            x[j >> 3] |= ((unsigned long long)v & 0xFFull) << (8 * (j & 7));
          }
        }
      }
    }
    if (high >> B) atomicOr(flags, 1u);                   // a token outside the alphabet (negative ones: sign bits)
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = pg_transpose8(x[i]);   // byte p of x[i]: bit p of tokens 8i .. 8i+7
#pragma unroll
    for (int p = 0; p < B; ++p) {
      const u32 w = (u32)((x[0] >> (8 * p)) & 0xFFull) | (u32)((x[1] >> (8 * p)) & 0xFFull) << 8 |
                    (u32)((x[2] >> (8 * p)) & 0xFFull) << 16 | (u32)((x[3] >> (8 * p)) & 0xFFull) << 24;
      words[sl * PG_PACK_LD + p * ng + g] = w;             // plane-major record order
    }
  }
  __syncthreads();
  // chunk arrays: lane = sequence, a whole uint4 per store; words past ng * B are zero
  const int nw = ng * B;
  for (int item = tid; item < PG_PACK_SEQS * nq; item += 256) {
    const int q = item / PG_PACK_SEQS, sl = item % PG_PACK_SEQS;
    uint4 v = *reinterpret_cast<const uint4 *>(&words[sl * PG_PACK_LD + 4 * q]);
    if (4 * q + 1 >= nw) v.y = 0;                          // (4 * q < nw always: nq = ceil(nw / 4))
    if (4 * q + 2 >= nw) v.z = 0;
    if (4 * q + 3 >= nw) v.w = 0;
    reinterpret_cast<uint4 *>(planes)[(long long)q * npad + s0 + sl] = v;
  }
  const int sl = tid & 63;
  const long long s = s0 + sl;
  if (tid < 64) {
    // Signature section (after the nq chunk arrays, 32 * npad bytes): the column operands of the filter MFMAs
    // (pg_mm.h), v_mfma_f32_32x32x64_f8f6f4 with FP4 elements: 1.0 (0x2) per set bit of the 54-bit signature,
    // 1.0 in the ten bias slots k = 54..63 (0 for padding sequences: they never pass); per 32 sequences one
    // 1 KiB block in fragment order: uint4 [tile][h * 32 + c] = elements k = 32h .. 32h+31 of sequence 32 * tile + c.
    u32 sigw[2] = {0, 0};                                   // plane 0, even / odd groups: the 64 bits behind the signature
    for (int g = 0; g < ng; ++g) sigw[g & 1] ^= words[sl * PG_PACK_LD + g];
    const unsigned long long sig = pg_sig54(sigw[0], sigw[1]);
    const u32 lo = (u32)sig, hi = (u32)(sig >> 32) | (s < n ? 0xFFC00000u : 0u);
    uint4 *e = reinterpret_cast<uint4 *>(planes + (long long)nq * npad * 4) + (s >> 5) * 64 + (s & 31);
    e[0] = make_uint4(pg_nib8(lo) << 1, pg_nib8(lo >> 8) << 1, pg_nib8(lo >> 16) << 1, pg_nib8(lo >> 24) << 1);
    e[32] = make_uint4(pg_nib8(hi) << 1, pg_nib8(hi >> 8) << 1, pg_nib8(hi >> 16) << 1, pg_nib8(hi >> 24) << 1);
  } else if (tid < 128) {
    // Fold section (after the signatures, 32 * npad bytes): two uint4 arrays, planes 0..3 and 4..7 of every
    // sequence's plane folds (XOR of each plane's group words; unused planes 0): the operands of the dense form's
    // folded-exact bound.
    u32 fold[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < B; ++p)
      for (int g = 0; g < ng; ++g) fold[p] ^= words[sl * PG_PACK_LD + p * ng + g];
    uint4 *f = reinterpret_cast<uint4 *>(planes + (long long)nq * npad * 4) + npad * 2;
    f[s] = make_uint4(fold[0], fold[1], fold[2], fold[3]);
    f[npad + s] = make_uint4(fold[4], fold[5], fold[6], fold[7]);
  }
}

// =======================================================================================
// exclusive scan (u32 counts or u8 flags -> i64), three small kernels
// =======================================================================================
#define PG_SCAN_TILE 2048   // elements per block (256 threads x 8)

template <typename T>
__device__ __forceinline__ long long scan_val(const T *in, long long i, long long n) {
  return i < n ? (long long)(in[i] != 0 ? (sizeof(T) == 1 ? 1 : in[i]) : 0) : 0;
}

__device__ __forceinline__ long long wave_incl_scan(long long v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    long long t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// block-wide exclusive scan of one value per thread (256 threads); returns the block total
__device__ __forceinline__ long long block_excl_scan(long long v, long long &total) {
  __shared__ long long wsum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long inc = wave_incl_scan(v, lane);
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  long long base = 0;
  for (int w = 0; w < wv; ++w) base += wsum[w];
  total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return base + inc - v;
}

template <typename T>
__global__ __launch_bounds__(256) void pg_scan_partials(const T *__restrict__ in, long long n, long long *partials) {
  const long long b0 = (long long)blockIdx.x * PG_SCAN_TILE;
  long long s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += scan_val(in, b0 + threadIdx.x * 8 + j, n);
  long long total;
  block_excl_scan(s, total);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void pg_scan_single(long long *partials, long long nb) {
  long long carry = 0;
  for (long long c0 = 0; c0 < nb; c0 += 256) {
    const long long i = c0 + threadIdx.x;
    const long long v = i < nb ? partials[i] : 0;
    long long total;
    const long long ex = block_excl_scan(v, total);
    if (i < nb) partials[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) partials[nb] = carry;
}

// MODE 0: out[i] = exclusive prefix (and out[n] = total); MODE 1: out[prefix] = i where in[i] != 0
template <typename T, int MODE>
__global__ __launch_bounds__(256) void pg_scan_apply(const T *__restrict__ in, long long n, const long long *partials,
                                                     long long nb, long long *out, long long *count) {
  const long long b0 = (long long)blockIdx.x * PG_SCAN_TILE;
  long long v[8], s = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { v[j] = scan_val(in, b0 + threadIdx.x * 8 + j, n); s += v[j]; }
  long long total;
  long long ex = block_excl_scan(s, total) + partials[blockIdx.x];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long long i = b0 + threadIdx.x * 8 + j;
    if (i < n) {
      if (MODE == 0) out[i] = ex;
      else if (v[j]) out[ex] = i;
    }
    ex += v[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (MODE == 0) out[n] = partials[nb];
    if (count) *count = partials[nb];
  }
}

// =======================================================================================
// fused 1xN indexing pass (one thread per sequence; position masks are bitmasks per group)
// =======================================================================================
template <int B>
__global__ __launch_bounds__(256) void pg_index_kernel(const u32 *__restrict__ planes, long long n, long long npad, int ng,
                                                       long long ref, const u32 *__restrict__ want, int posMode,
                                                       const u32 *__restrict__ posMask, const u32 *__restrict__ notMask,
                                                       unsigned char *distOut, u64 *hist, unsigned char *flags) {
  __shared__ u32 lh[256];
  lh[threadIdx.x] = 0;
  __syncthreads();
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s < n) {
    u32 d = 0, anyP = 0, anyNot = 0;
    bool allP = true;
    for (int g = 0; g < ng; ++g) {
      u32 t = 0;
#pragma unroll
      for (int p = 0; p < B; ++p) {
        const int w = p * ng + g;
        const long long base = (long long)(w >> 2) * npad;
        t |= planes[(base + s) * 4 + (w & 3)] ^ planes[(base + ref) * 4 + (w & 3)];
      }
      d += __builtin_popcount(t);
      if (posMode) {
        const u32 pm = posMask[g], nm = notMask[g];
        anyP |= t & pm;
        allP = allP && ((t & pm) == pm);
        anyNot |= t & nm;
      }
    }
    if (distOut) distOut[s] = (unsigned char)d;
    if (hist) atomicAdd(&lh[d & 255u], 1u);
    if (flags) {
      bool ok = want ? ((want[(d >> 5) & 7u] >> (d & 31u)) & 1u) != 0 : true;
      if (posMode == 1) ok = ok && (anyP != 0) && (anyNot == 0);
      if (posMode == 2) ok = ok && allP && (anyNot == 0);
      flags[s] = ok ? 1 : 0;
    }
  }
  __syncthreads();
  if (hist && lh[threadIdx.x]) atomicAdd((unsigned long long *)&hist[threadIdx.x], (unsigned long long)lh[threadIdx.x]);
}

// =======================================================================================
// CSR consumers: per-row reductions the graph analytics need
//   deg[r]  = sum_j w_rj            (degree, prograph/prograph.py:797-822)
//   sf[r]   = sum_j f[col_j]        (local_variance, :924-946:  mean_j (f_r - f_j) = f_r - sf/cnt)
//   swf[r]  = sum_j w_rj f[col_j]   (dirichlet, :899-922:  f^T L f = sum_r f_r (deg_r f_r - swf_r))
// one wave per row, coalesced reads of the row's slice, DPP/shuffle tree reduction.
// An entry with a negative column (an empty kNN slot) is no edge: it enters no sum, and neither f nor colsum is touched.
// =======================================================================================
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

__global__ __launch_bounds__(256) void pg_csr_row_stats_kernel(const long long *__restrict__ indptr,
                                                               const int *__restrict__ indices,
                                                               const unsigned char *__restrict__ w8,
                                                               const float *__restrict__ wf, long long nrows,
                                                               long long row0, const double *__restrict__ f, double *deg,
                                                               double *sf, double *swf, double *selfw, double *colsum) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nrows) return;
  const long long a = indptr[row], b = indptr[row + 1];
  double d = 0, s1 = 0, s2 = 0, sw = 0;
  for (long long e = a + lane; e < b; e += 64) {
    const double w = w8 ? (double)w8[e] : (wf ? (double)wf[e] : 1.0);
    const int col = indices[e];
    if (col < 0) continue;                                // an empty kNN slot: no edge, nothing is read or added for it
    const double fj = f ? f[col] : 0.0;
    d += w; s1 += fj; s2 += w * fj;
    if (col == row0 + row) sw += w;                       // the row's own node among its neighbours
    if (colsum) atomicAdd(&colsum[col], w);               // in-degree (column sums of the adjacency)
  }
  d = wave_sum(d); s1 = wave_sum(s1); s2 = wave_sum(s2); sw = wave_sum(sw);
  if (lane == 0) {
    if (deg) deg[row] = d;
    if (sf) sf[row] = s1;
    if (swf) swf[row] = s2;
    if (selfw) selfw[row] = sw;
  }
}

// =======================================================================================
// host side of the ABI
// =======================================================================================
// `l` may be the packed width rounded up to whole 32-token groups (256 for 8 groups); only
// pg_pack_planes, which sees the real tokens, enforces L <= 255 (a distance must fit uint8).
static int check_l(int l, int bits = 8, bool exact = false) {
  if (l <= 0) return pg_fail(PG_E_BADARG, "sequence length must be positive");
  const int maxg = bits == 5 ? PG_MAX_L_5BIT / 32 + 1 : PG_MAX_L / 32;
  if ((l + 31) / 32 > maxg || (exact && l > (bits == 5 ? PG_MAX_L_5BIT : PG_MAX_L)))
    return pg_fail(PG_E_TOOLONG, "sequence length exceeds the native limit (128 tokens, 255 with 5 bit planes)");
  return 0;
}
static int check_bits(int b) {
  if (b != PG_BITS_5 && b != PG_BITS_8) return pg_fail(PG_E_BADARG, "bits must be 5 or 8");
  return 0;
}

// comp(d, eps) & (d >= dmin) as an integer interval [lo, lo+span]; an empty interval is encoded
// so that (d - lo) <= span is false for every d in 0..255.  dmin = 1: the graphs (pairs with d = 0 are
// excluded); dmin = 0: queries (pg_query_eps_*)
static void eps_interval(int cmp, double eps, u32 *lo, u32 *span, long long dmin = 1) {
  const long long INF = 1000000;
  long long l = dmin, h = INF;
  switch (cmp) {
    case PG_CMP_LE: h = (long long)floor(eps); break;
    case PG_CMP_LT: h = (long long)ceil(eps) - 1; break;
    case PG_CMP_EQ:
      if (floor(eps) == eps) { l = (long long)eps; h = (long long)eps; } else { l = 1; h = 0; }
      break;
    case PG_CMP_GE: l = (long long)ceil(eps); break;
    case PG_CMP_GT: l = (long long)floor(eps) + 1; break;
  }
  if (l < dmin) l = dmin;
  if (h > INF) h = INF;
  if (h < l) { *lo = 0xFFFFFF00u; *span = 0; return; }
  *lo = (u32)l;
  *span = (u32)(h - l);
}

// ---------------------------------------------------------------------------------------
// Data probe + decision (no host round trip): pg_probe_kernel counts, for PG_PROBE_ROWS sample rows of the launch, the
// columns nearer than the kNN cap and the columns inside the eps interval; pg_decide_kernel turns them into the gate
// words the alternative kernels of the launch test at their start (NsqParams::gate) - and zeroes the workspace's counter
// block for the launch to come, which then needs no fill of its own (pass_counter):
//   gate[0]  kNN engine: 0 = MFMA engine, 1 = VALU engine.  Unclustered data (fewer than half of the sample rows have
//            k + 1 columns below the cap: the signature filter never gets a useful bound, every distance is needed)
//            runs ~8 % faster on the VALU engine's direct form (profiles/r03_engine_landscape.txt: random N = 200k);
//            2 = MFMA engine with 32-row passes although 64-row passes were planned: ONE cluster (more than half of
//            all pairs below the cap) lives in the folded form, where the finer pass granularity wins (11.7 vs 12.5 ms)
//   gate[1]  whole-square eps graph: 0 = every unordered pair once (symmetric slots), 1 = rectangular VALU sweep.
//            Dense graphs (more than 4 % of all pairs match) pay more for the symmetric path's atomics and
//            unsorted back parts than it saves (one cluster, eps <= 2: 39.6 vs 29.4 ms)
//   gate[2]  (not the probe's: the merge of a symmetric kNN sweep, pg_knn_sym_merge_kernel, writes it) what the
//            rectangular kNN launches and pg_knn_rows_kernel of that call test instead of gate[0]: gate[0]'s value where
//            the probe chose another engine or instance, 0 where the sweep evicted more rows than its limit (the
//            rectangular launch runs), 3 where its results stand (pg_knn_rows_kernel alone runs, for its evicted rows)
// ---------------------------------------------------------------------------------------
// (PG_PROBE_ROWS, PG_PROBE_WAVES, PG_PROBE_MIN_N: pg_plan.h)
// one workgroup: 16 threads per sample row (a quarter wave) sum the row's per-wave counts, the wave of a row then the
// workgroup combine the verdicts
__global__ __launch_bounds__(1024) void pg_decide_kernel(const u32 *counts, int nsample, int wavesPerRow, u32 need, long long ncols,
                                                          int force, u32 *gate, u32 *line, int lineWords, SymPlanArgs ride) {
  // the workgroups behind the first: the plan of the symmetric sweep this launch is followed by (sym_plan_workgroup; their
  // writes - the plan, pieceStart, the zeroed counts of delivered keys - and the decision's are disjoint regions)
  if (blockIdx.x > 0) { sym_plan_workgroup(blockIdx.x - 1u, gridDim.x - 1u, ride); return; }
  __shared__ u32 sClustered[16];
  __shared__ unsigned long long sEps[16], sNear[16];
  const int tid = threadIdx.x, s = tid >> 4, sub = tid & 15;
  if (tid < lineWords) line[tid] = 0u;                     // the counter block: nothing reads it before the launch behind this one
  u32 nearS = 0, epsS = 0;
  if (s < nsample)
    for (int w = sub; w < wavesPerRow; w += 16) {
      nearS += counts[2 * (s * wavesPerRow + w)];
      epsS += counts[2 * (s * wavesPerRow + w) + 1];
    }
  for (int o = 8; o > 0; o >>= 1) {
    nearS += (u32)__shfl_xor((int)nearS, o);
    epsS += (u32)__shfl_xor((int)epsS, o);
  }
  // (counts are over every PG_PROBE_STRIDE-th tile)
  u32 clustered = (sub == 0 && s < nsample && nearS * PG_PROBE_STRIDE >= need) ? 1u : 0u;
  unsigned long long eps = (sub == 0 && s < nsample) ? (unsigned long long)epsS * PG_PROBE_STRIDE : 0ull;
  unsigned long long nearAll = (sub == 0 && s < nsample) ? (unsigned long long)nearS * PG_PROBE_STRIDE : 0ull;
  for (int o = 32; o > 0; o >>= 1) {
    clustered += (u32)__shfl_xor((int)clustered, o);
    eps += (unsigned long long)__shfl_xor((long long)eps, o);
    nearAll += (unsigned long long)__shfl_xor((long long)nearAll, o);
  }
  if ((tid & 63) == 0) { sClustered[tid >> 6] = clustered; sEps[tid >> 6] = eps; sNear[tid >> 6] = nearAll; }
  __syncthreads();
  if (tid == 0) {
    clustered = 0; eps = 0; nearAll = 0;
    for (int i = 0; i < 16; ++i) { clustered += sClustered[i]; eps += sEps[i]; nearAll += sNear[i]; }
    const bool oneCluster = 2ull * nearAll > (unsigned long long)nsample * (unsigned long long)ncols;
    gate[0] = force >= 0 ? (u32)(force & 1) + ((force & 4) ? 2u : 0u) : (2u * clustered >= (u32)nsample ? (oneCluster ? 2u : 0u) : 1u);
    gate[1] = force >= 0 ? (u32)((force >> 1) & 1) : (eps * 25ull > (unsigned long long)nsample * (unsigned long long)ncols ? 1u : 0u);
  }
}
// kNN of rows swept in column pieces (NsqParams::mmPieces): a row's `pieces` (<= 16) sorted lists of k + 1 keys each -> its
// k + 1 smallest keys, ranks 1..k written out (the reference drops sorted rank 0, prograph/prograph.py:761-763).  Sixteen
// lanes per row, lane b holds the head of list b: k + 1 rounds of "smallest head wins and advances" (keys are
// distance << 24 | column: unique, except 0xFFFFFFFF = no entry).  Four rows per wave.
// A piece's list is exact below the optimistic cap only (NsqParams::mmPieces): a row whose merged (k+1)-th distance is
// not below `cap` joins the evicted rows (NsqParams::mmEvict: pg_knn_rows_kernel finishes them).
__global__ __launch_bounds__(PG_WG_THREADS) void pg_knn_merge_kernel(const u32 *partial, long long nrows, int pieces, int k, int *idx,
                                                                     unsigned char *dist, u32 cap, u32 *evictCount, u32 *evictRows,
                                                                     long long rowAbs0, const u32 *gate, u32 gateMask) {
  __shared__ u32 keys[PG_WG_WAVES][4][16 * PG_MM_KL];
  if (gate && !((gateMask >> __builtin_nontemporal_load(gate)) & 1u)) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, b = lane & 15;
  const long long row0 = ((long long)blockIdx.x * PG_WG_WAVES + wv) * 4;
  if (row0 >= nrows) return;                               // (whole wave; no workgroup barrier below)
  const int k1 = k + 1, n = pieces * k1;
  for (int r = 0; r < 4; ++r)
    if (row0 + r < nrows)
      for (int e = lane; e < n; e += 64) keys[wv][r][e] = partial[(row0 + r) * n + e];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const long long row = row0 + g;
  const bool mine = row < nrows && b < pieces;
  int pos = 0;
  u32 head = mine ? keys[wv][g][b * k1] : 0xFFFFFFFFu;
  for (int r = 0; r <= k; ++r) {
    u32 m = head;
    for (int o = 8; o > 0; o >>= 1) {
      const u32 x = (u32)__shfl_xor((int)m, o, 16);
      m = x < m ? x : m;
    }
    if (b == 0 && row < nrows) {
      if (r >= 1) {
        idx[row * k + r - 1] = m == 0xFFFFFFFFu ? -1 : (int)(m & 0x00FFFFFFu);
        dist[row * k + r - 1] = (unsigned char)(m >> 24);
      }
      if (r == k && (m >> 24) >= cap) evictRows[atomicAdd(evictCount, 1u)] = (u32)(rowAbs0 + row);   // (0xFFFFFFFF, no entry, reads 255)
    }
    if (mine && head == m && m != 0xFFFFFFFFu) {           // the winner (unique key) moves on in its list
      ++pos;
      head = pos < k1 ? keys[wv][g][b * k1 + pos] : 0xFFFFFFFFu;
    }
  }
}

// kNN of the symmetric sweep (pg_mm_knn_sym_kernel): a row's records - one per piece of its block, passes
// pieceStart[block] .. pieceStart[block + 1], PG_MM_KL keys each with the sorted list of k + 1 keys at the end - and the
// keys delivered to it -> its k + 1 smallest keys in (distance << 24 | index) order, the order of the rectangular sweep;
// ranks 1..k written out.  Sixteen lanes per row, four rows per wave, sixteen rows per workgroup and trip: one GROUP of
// receiver rows, whose delivered keys are one append log (pg_plan.h: sym_entry; word 16 g of lowCount counts it).
// Binning: the workgroup reads the log coalesced - min(count, sym_group_cap) entries, all 256 threads - and puts every entry,
// expanded to distance << 24 | sender row again, into its row's bin of capL keys in LDS; a returning LDS add on the row's
// count gives the place, places from capL on are not stored, the count runs on.  Behind a barrier lane b takes its bin's
// entries into registers; behind another the rows' records are staged in the SAME LDS block (the bins have left it: 20 KB
// a workgroup, not 36, and 7 waves per SIMD, not 4: 118 -> 106 us at cfg3); the next trip's first barrier stands behind the
// last read of them.  Three barriers a trip; the counts are two sets in turn (a trip zeroes the next one's, whose last
// readers passed the trip before's third barrier) - and every wave of a workgroup makes the same trips (the bound is the
// workgroup's first row), so the barrier in front of the ticket is reached by all of them.
// The loads of the block's passes and of lane b's record b (five 16-byte loads) are issued in front of the binning.
// Selection: lane b takes entries b, b + 16, ... of its row's bin into sixteen registers and sorts them once (a network of
// 63 compare-exchanges), then k + 1
// rounds of "smallest head wins and advances" over the sixteen lanes' two heads - list b's, a pointer into the staged
// record, and the lane's delivered keys', of which a WINDOW of W (template parameter: 4; 1 and 2 for tests,
// PG_KNN_SYM_MERGE_WINDOW) moves down one register when the head wins, refilled from the registers behind it in a cold
// branch (pg_plan.h: sym_window_pop, sym_window_refill - a lane wins about once a trip at cfg3, and the whole list's
// shift was 16 of a round's ~35 instructions): one reduction a round, nothing is
// scanned twice (keys are unique; equal heads advance together; 0xFFFFFFFF = no entry).
// Every list is complete below the cap only: a row whose (k+1)-th distance is not below it, or whose bin overflowed, joins
// the evicted rows (pg_knn_rows_kernel finishes them) - and so do all sixteen rows of a group whose LOG overflowed: entries
// were lost and nobody knows whose (some row of such a group is over capL anyway).
// The decision behind the merge is taken by the workgroup that finishes last (a ticket: `ticket`, a zeroed word of the
// counter block, left at 0 again): too many evicted rows (clusters much larger than the slots of delivered keys, data
// without neighbours below the cap) - the rectangular launch behind this kernel runs instead and starts from no evicted
// rows.  gate2: what the launches behind test: 3 = the symmetric sweep stands (only pg_knn_rows_kernel runs), else the
// probe's word (0 without one).  Workgroups that have no rows, or leave at the gate, take their ticket all the same.
// Resource line (hipcc -O3, gfx950; W = 1, 2 and 4 alike): 72 VGPRs, 75 SGPRs, no scratch, LDS 20 608 B, 7 waves per SIMD
// (profiles/r17_knn_sym_group_delivery.json has the builds measured: the parent's per-row slots 81 us, bins beside the records
// 118, the whole-list shift 106; profiles/r18_knn_sym_merge_window.json: 112 -> 94 us with the window, SQ_INSTS_VALU 3.92e7 -> 3.24e7).
// lane i of a row of sixteen reads lane (i + N) & 15
#define PG_SYM_ROR(x, N) ((u32)__builtin_amdgcn_update_dpp(0, (int)(x), 0x120 + (N), 0xF, 0xF, false))
#define PG_SYM_CE(a, b) { const u32 x_ = a, y_ = b; a = x_ < y_ ? x_ : y_; b = x_ < y_ ? y_ : x_; }
template <int W>
__global__ __launch_bounds__(PG_WG_THREADS) __attribute__((amdgpu_waves_per_eu(7, 8))) void pg_knn_sym_merge_kernel(const u32 *partial, const u32 *pieceStart, const u32 *lowCount,
                                                                         const u32 *lowKeys, u32 capL, int rowBits, long long nrows, int k, int *idx,
                                                                         unsigned char *dist, u32 cap, u32 *evictCount, u32 *evictRows,
                                                                         const u32 *gate, u32 gateMask, u32 *gate2, u32 *ticket, u32 limit) {
  constexpr int kRec = PG_MM_KL, kOwn = PG_SYM_MAX_PIECES * kRec, kLane = PG_SYM_MAX_CAPL / 16;
  static_assert(kRec == 20 && kLane == 16, "records of whole uint4; sixteen delivered keys a lane");
  // one LDS block in two roles a trip: the group's bins (per row its delivered keys, as they arrive) while the log is read,
  // then - the bins are in registers - the rows' records
  __shared__ __attribute__((aligned(16))) u32 keys[PG_WG_WAVES][4][kOwn];
  static_assert(4 * PG_WG_WAVES * PG_SYM_MAX_CAPL <= PG_WG_WAVES * 4 * kOwn, "the bins fit the records' block");
  u32 (*bins)[PG_SYM_MAX_CAPL] = reinterpret_cast<u32 (*)[PG_SYM_MAX_CAPL]>(&keys[0][0][0]);
  __shared__ u32 binCount[2][4 * PG_WG_WAVES];               // how many keys arrived for a row (two sets: trips in turn)
  const u32 gv = gate ? __builtin_nontemporal_load(gate) : 0u;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, b = lane & 15;
  const bool open = !gate || ((gateMask >> gv) & 1u);
  if (threadIdx.x < 4 * PG_WG_WAVES) binCount[0][threadIdx.x] = 0u;
  int trip = 0;
  // a trip's header - the passes of its block, pieceStart[blk] and pieceStart[blk + 1], and the group's count - is read a
  // trip ahead (the first one here)
  u32 hs0 = 0u, hs1 = 0u, hlogged = 0u;
  if (open && (long long)blockIdx.x * (4 * PG_WG_WAVES) < nrows) {
    const long long f0 = (long long)blockIdx.x * (4 * PG_WG_WAVES);
    hs0 = pieceStart[f0 >> 6]; hs1 = pieceStart[(f0 >> 6) + 1]; hlogged = lowCount[f0];
  }
  // (whole workgroups; the grid is a few workgroups a CU, every one takes a group of sixteen rows in turns: few tickets on one word)
  for (long long first = (long long)blockIdx.x * (4 * PG_WG_WAVES); open && first < nrows; first += (long long)gridDim.x * (4 * PG_WG_WAVES), trip ^= 1) {
    const int k1 = k + 1, off = kRec - k1;
    // (sixteen consecutive rows from a multiple of sixteen: one block, first >> 6)
    const long long row = first + 4 * wv + g;
    const bool mine = row < nrows;
    const long long rowIn = mine ? row : first;              // (idle lanes read the group's first row: in bounds, unused)
    // level 1: the block's passes and the group's count; then record b - unconditional loads from addresses inside the
    // workspace (a lane without a piece reads record 0 of its block), masked afterwards
    const u32 s0 = hs0, s1 = hs1;
    const u32 logged = (u32)__builtin_amdgcn_readfirstlane((int)hlogged);
    u32 np = s1 - s0;
    np = np > PG_SYM_MAX_PIECES ? PG_SYM_MAX_PIECES : np;
    u32 *own = &keys[wv][g][0];
    const bool has = mine && b < (int)np;
    const uint4 *rec = reinterpret_cast<const uint4 *>(partial) + (((long long)s0 + (b < (int)np ? b : 0)) * 64 + (rowIn & 63)) * (kRec / 4);
    const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3], r4 = rec[4];
    // the group's log into the rows' bins
    const u32 capG = sym_group_cap((u32)nrows, (u32)first, capL);
    const u32 nlog = logged < capG ? logged : capG;
    const u32 *log = lowKeys + first * (long long)capL;
    __syncthreads();                                         // (the last trip's records are read; this trip's counts are zero)
    for (u32 e0 = threadIdx.x; e0 < nlog; e0 += 4 * PG_WG_THREADS) {   // (four loads of a thread in flight)
      u32 en[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) en[j] = e0 + j * PG_WG_THREADS < nlog ? log[e0 + j * PG_WG_THREADS] : 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e0 + j * PG_WG_THREADS < nlog) {
          const u32 place = sym_entry_place(en[j]);
          const u32 at = atomicAdd(&binCount[trip][place], 1u);
          if (at < capL) bins[place][at] = sym_entry_key(en[j], rowBits);
        }
      }
    }
    if (threadIdx.x < 4 * PG_WG_WAVES) binCount[trip ^ 1][threadIdx.x] = 0u;   // (last read before the last trip's third barrier)
    __syncthreads();
    // lane b: entries b, b + 16, ... of its row's bin
    // (the sixteen delivered keys of a lane are indexed by constants only: every one stays in its register)
    const u32 cnt = mine ? binCount[trip][4 * wv + g] : 0u;
    const int nl = (int)(cnt < capL ? cnt : capL);
    const u32 *low = &bins[4 * wv + g][b];
    u32 d[16];
#define PG_SYM_BIN(j, d) d = 16 * j + b < nl ? low[16 * j] : 0xFFFFFFFFu;
    PG_SYM_BIN(0, d[0]) PG_SYM_BIN(1, d[1]) PG_SYM_BIN(2, d[2]) PG_SYM_BIN(3, d[3]) PG_SYM_BIN(4, d[4]) PG_SYM_BIN(5, d[5]) PG_SYM_BIN(6, d[6]) PG_SYM_BIN(7, d[7])
    PG_SYM_BIN(8, d[8]) PG_SYM_BIN(9, d[9]) PG_SYM_BIN(10, d[10]) PG_SYM_BIN(11, d[11]) PG_SYM_BIN(12, d[12]) PG_SYM_BIN(13, d[13]) PG_SYM_BIN(14, d[14]) PG_SYM_BIN(15, d[15])
#undef PG_SYM_BIN
    __syncthreads();                                         // (the bins are in registers: the block takes the records)
    {
      uint4 *st = reinterpret_cast<uint4 *>(own + b * kRec);  // (a lane without a piece stages what it read: never its head)
      st[0] = r0; st[1] = r1; st[2] = r2; st[3] = r3; st[4] = r4;
    }
    // the lane's delivered keys in ascending order (no entries last: Batcher's odd-even merge sort of sixteen); rows of
    // up to sixteen keys hold one a lane, as it stands
    if (__builtin_amdgcn_ballot_w64(nl > 16) != 0) {
      PG_SYM_CE(d[0], d[1]) PG_SYM_CE(d[2], d[3]) PG_SYM_CE(d[4], d[5]) PG_SYM_CE(d[6], d[7]) PG_SYM_CE(d[8], d[9]) PG_SYM_CE(d[10], d[11]) PG_SYM_CE(d[12], d[13]) PG_SYM_CE(d[14], d[15])
      PG_SYM_CE(d[0], d[2]) PG_SYM_CE(d[1], d[3]) PG_SYM_CE(d[4], d[6]) PG_SYM_CE(d[5], d[7]) PG_SYM_CE(d[8], d[10]) PG_SYM_CE(d[9], d[11]) PG_SYM_CE(d[12], d[14]) PG_SYM_CE(d[13], d[15])
      PG_SYM_CE(d[1], d[2]) PG_SYM_CE(d[5], d[6]) PG_SYM_CE(d[9], d[10]) PG_SYM_CE(d[13], d[14]) PG_SYM_CE(d[0], d[4]) PG_SYM_CE(d[1], d[5]) PG_SYM_CE(d[2], d[6]) PG_SYM_CE(d[3], d[7])
      PG_SYM_CE(d[8], d[12]) PG_SYM_CE(d[9], d[13]) PG_SYM_CE(d[10], d[14]) PG_SYM_CE(d[11], d[15]) PG_SYM_CE(d[2], d[4]) PG_SYM_CE(d[3], d[5]) PG_SYM_CE(d[10], d[12]) PG_SYM_CE(d[11], d[13])
      PG_SYM_CE(d[1], d[2]) PG_SYM_CE(d[3], d[4]) PG_SYM_CE(d[5], d[6]) PG_SYM_CE(d[9], d[10]) PG_SYM_CE(d[11], d[12]) PG_SYM_CE(d[13], d[14]) PG_SYM_CE(d[0], d[8]) PG_SYM_CE(d[1], d[9])
      PG_SYM_CE(d[2], d[10]) PG_SYM_CE(d[3], d[11]) PG_SYM_CE(d[4], d[12]) PG_SYM_CE(d[5], d[13]) PG_SYM_CE(d[6], d[14]) PG_SYM_CE(d[7], d[15]) PG_SYM_CE(d[4], d[8]) PG_SYM_CE(d[5], d[9])
      PG_SYM_CE(d[6], d[10]) PG_SYM_CE(d[7], d[11]) PG_SYM_CE(d[2], d[4]) PG_SYM_CE(d[3], d[5]) PG_SYM_CE(d[6], d[8]) PG_SYM_CE(d[7], d[9]) PG_SYM_CE(d[10], d[12]) PG_SYM_CE(d[11], d[13])
      PG_SYM_CE(d[1], d[2]) PG_SYM_CE(d[3], d[4]) PG_SYM_CE(d[5], d[6]) PG_SYM_CE(d[7], d[8]) PG_SYM_CE(d[9], d[10]) PG_SYM_CE(d[11], d[12]) PG_SYM_CE(d[13], d[14])
    }
    // heads of the own list (a pointer: the lane reads what it staged itself) and of the delivered keys (d0); lane r - 1
    // keeps rank r (ranks from 17 on: lane 0 writes)
    // the next trip's header: three words, the same for the whole workgroup, asked for here so that the records' addresses
    // and the log's bound do not wait for a round trip at the top of the trip (a last trip asks for nothing)
    {
      const long long next = first + (long long)gridDim.x * (4 * PG_WG_WAVES);
      // (a zero the compiler cannot see in the count's address: a load it knows to be uniform is read into an SGPR where
      //  it is issued, and the wave would wait for it here, in front of the rounds; the trip's top reads the first lane)
      u32 zero = 0u;
      asm volatile("" : "+v"(zero));
      if (next < nrows) { hs0 = pieceStart[next >> 6]; hs1 = pieceStart[(next >> 6) + 1]; hlogged = lowCount[next + zero]; }
    }
    int pos = 0, used = 0;
    u32 head = has ? own[b * kRec + off] : 0xFFFFFFFFu, res = 0xFFFFFFFFu;
    for (int r = 0; r <= k; ++r) {
      u32 m = head < d[0] ? head : d[0], x;
      x = PG_SYM_ROR(m, 8); m = x < m ? x : m;
      x = PG_SYM_ROR(m, 4); m = x < m ? x : m;
      x = PG_SYM_ROR(m, 2); m = x < m ? x : m;
      x = PG_SYM_ROR(m, 1); m = x < m ? x : m;
      const bool any = m != 0xFFFFFFFFu;
      if (any && head == m) {                                // the winner moves on in its list
        ++pos;
        head = pos < k1 ? own[b * kRec + off + pos] : 0xFFFFFFFFu;
      }
      // ... or the window of its delivered keys moves down a register (pg_plan.h: sym_window_pop); a lane whose window has
      // run empty takes the W keys behind it - the cold path, where some lane of the wave won W times since its last refill
      sym_window_pop<W>(d, used, any && d[0] == m);
      if (__builtin_amdgcn_ballot_w64(sym_window_empty<W>(used)) != 0) sym_window_refill<W>(d, used);
      if (b == r - 1) res = m;
      if (b == 0 && mine) {
        if (r > 16) {
          idx[row * k + r - 1] = m == 0xFFFFFFFFu ? -1 : (int)(m & 0x00FFFFFFu);
          dist[row * k + r - 1] = (unsigned char)(m >> 24);
        }
        if (r == k && ((m >> 24) >= cap || cnt > capL || logged > capG)) evictRows[atomicAdd(evictCount, 1u)] = (u32)row;   // (0xFFFFFFFF, no entry, reads 255)
      }
    }
    if (mine && b < k) {
      idx[row * k + b] = res == 0xFFFFFFFFu ? -1 : (int)(res & 0x00FFFFFFu);
      dist[row * k + b] = (unsigned char)(res >> 24);
    }
  }
  __syncthreads();                                           // (every wave of the workgroup: its rows' evictions are counted)
  // The ticket is a RELAXED add, and no fence stands beside it.  What the workgroup that draws the last one reads of the
  // others is the count of evicted rows alone, and that word is only ever touched by agent-scope atomic read-modify-writes,
  // which execute at the memory side, not in an XCD's L2: (1) every evict add above is a returning atomic whose value is
  // used - the index of the store beside it - so it has been performed when its wave arrives at the barrier; (2) thread
  // 0's ticket add is issued behind that barrier, so it is performed after every evict add of its workgroup; (3) the last
  // ticket is drawn after all others were performed; (4) the decider reads the count with a read-modify-write of its own,
  // issued after its ticket came back and before any of its stores (the ticket's word shares the count's 128-byte line).
  // That read is an add of a zero the compiler cannot see: an add of the constant 0 is folded into a load (`global_load_dword
  // ... sc1`, served by an L2 that may have kept the line); in the ISA it is `global_atomic_add ... sc0`, the third atomic
  // of the kernel.  Nothing cached takes part, so there is nothing to release or to acquire.  The results, evictRows and the
  // words the decider stores (the ticket back to 0, gate2, the count) are read by the launches behind this one only.
  // (The release/acquire pair - an L2 write-back and an L1 invalidate per workgroup, 2048 of them - cost 50 us at cfg3.)
  if (threadIdx.x == 0) {
    if (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) {
      u32 zero = 0u;
      asm volatile("" : "+v"(zero));                         // (opaque: keeps the add an atomic instruction)
      const u32 evictedRows = __hip_atomic_fetch_add(evictCount, zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *ticket = 0u;
      if (gv != 0u) *gate2 = gv;
      else if (evictedRows > limit) { *evictCount = 0u; *gate2 = 0u; }
      else *gate2 = 3u;
    }
  }
}

typedef int (*probe_fn)(int, const ProbeParams &, hipStream_t);
typedef int (*knn_rows_fn)(int, const KnnRowsParams &, int, hipStream_t);
static const knn_rows_fn kKnnRows[8] = {pg_launch_knn_rows_g1, pg_launch_knn_rows_g2, pg_launch_knn_rows_g3, pg_launch_knn_rows_g4,
                                        pg_launch_knn_rows_g5, pg_launch_knn_rows_g6, pg_launch_knn_rows_g7, pg_launch_knn_rows_g8};
static const probe_fn kProbe[8] = {pg_launch_probe_g1, pg_launch_probe_g2, pg_launch_probe_g3, pg_launch_probe_g4,
                                   pg_launch_probe_g5, pg_launch_probe_g6, pg_launch_probe_g7, pg_launch_probe_g8};
// (whether a launch is probed: probe_enabled, pg_plan.h; PG_GATE_FORCE=<bits>: the decision is forced (tests): bit 0 gate[0], bit 1 gate[1])
// zeroes workspace[0, 576) (the counter block: pass_counter issues no fill behind a probe) and fills workspace[576, ...):
// returns the gate words through *gate
static int run_probe(const NsqParams &e, int l, int bits, u32 near, u32 lo, u32 span, u32 need, void *workspace, hipStream_t s,
                     const PgKnobs &kn, const u32 **gate, const SymPlanArgs *ride = nullptr) {
  if (!workspace) return pg_fail(PG_E_BADARG, "workspace required (pg_workspace_bytes)");
  u32 *gates = (u32 *)((char *)workspace + PG_WS_GATES), *counts = (u32 *)((char *)workspace + PG_WS_COUNTS);
  ProbeParams pp;
  pp.rowPlanes = e.rowPlanes; pp.colPlanes = e.colPlanes; pp.rowNpad = e.rowNpad; pp.colNpad = e.colNpad;
  pp.row0 = e.row0; pp.nrows = e.nrows; pp.ncols = e.ncols;
  pp.nsample = e.nrows < PG_PROBE_ROWS ? (int)e.nrows : PG_PROBE_ROWS;
  pp.wavesPerRow = PG_PROBE_WAVES;
  if (kn.probeS.v > 0) pp.nsample = (int)kn.probeS.v;       // (experiments)
  if (kn.probeW.v > 0) pp.wavesPerRow = (int)kn.probeW.v;
  pp.near = near; pp.lo = lo; pp.span = span; pp.counts = counts;
  if (int rc = pg_launched(kProbe[pg_ngroups(l) - 1](bits, pp, s), "pg_probe_kernel")) return rc;
  const int force = (int)kn.gateForce.v;
  // (counts of a short sample: pg_decide_kernel reads counts[nsample + s] - same layout as the probe wrote)
  static_assert(PG_WS_GATES / 4 <= 1024, "pg_decide_kernel zeroes one word per thread");
  // (ride: the plan of the symmetric sweep behind this launch, in workgroups of its own - KnnPlan::symPlanRides)
  const SymPlanArgs none = {};
  pg_decide_kernel<<<dim3(1u + (ride ? ride->grid : 0u)), dim3(1024), 0, s>>>(counts, pp.nsample, pp.wavesPerRow, need, e.ncols, force, gates, (u32 *)workspace,
                                                                              PG_WS_GATES / 4, ride ? *ride : none);   // (PG_PROBE_ROWS <= 64)
  if (int rc = pg_launched("pg_decide_kernel")) return rc;
  *gate = gates;
  return 0;
}

typedef int (*nsq_fn)(int, int, const NsqParams &, int, hipStream_t);
typedef int (*dense_fn)(int, const DenseParams &, hipStream_t);
typedef int (*compact_fn)(int, const CompactParams &, hipStream_t);
typedef int (*occ_fn)(int, int);
static const occ_fn kNsqOcc[8] = {pg_occ_nsq_g1, pg_occ_nsq_g2, pg_occ_nsq_g3, pg_occ_nsq_g4,
                                  pg_occ_nsq_g5, pg_occ_nsq_g6, pg_occ_nsq_g7, pg_occ_nsq_g8};
// resident waves per SIMD (= workgroups per CU) of an engine instance, asked once from the runtime
static int nsq_occupancy(int groups, int mode, int bits) {
  static std::atomic<int> cache[8][3][2];                  // (a property of the code object: the same on every gfx950)
  std::atomic<int> &c = cache[groups - 1][mode][bits == 8];
  int v = c.load(std::memory_order_relaxed);
  if (v == 0) {
    const int n = kNsqOcc[groups - 1](mode, bits);
    v = n < 1 ? 4 : (n > 8 ? 8 : n);
    c.store(v, std::memory_order_relaxed);
  }
  return v;
}
static const nsq_fn kNsq[8] = {pg_launch_nsq_g1, pg_launch_nsq_g2, pg_launch_nsq_g3, pg_launch_nsq_g4,
                               pg_launch_nsq_g5, pg_launch_nsq_g6, pg_launch_nsq_g7, pg_launch_nsq_g8};
static const dense_fn kDense[8] = {pg_launch_dense_g1, pg_launch_dense_g2, pg_launch_dense_g3, pg_launch_dense_g4,
                                   pg_launch_dense_g5, pg_launch_dense_g6, pg_launch_dense_g7, pg_launch_dense_g8};
static const compact_fn kCompact[8] = {pg_launch_compact_g1, pg_launch_compact_g2, pg_launch_compact_g3,
                                       pg_launch_compact_g4, pg_launch_compact_g5, pg_launch_compact_g6,
                                       pg_launch_compact_g7, pg_launch_compact_g8};

// The row split of a VALU-engine launch (plan_rows, pg_plan.h) goes into its parameters
static void set_rows_plan(NsqParams *p, int *grid, const PassPlan &pl, const PgKnobs &kn) {
  if (kn.debugPlan.set) fprintf(stderr, "[pg plan] rows=%lld occ=%d rows_per_wave=%lld waves=%lld\n", (long long)p->nrows, pl.occ, (long long)pl.rowsPerWave, pl.passes);
  p->rowsPerWave = pl.rowsPerWave; p->rowsPerPass = pl.rowsPerPass;
  *grid = pl.grid;
}
// ... planned here, for the device of the call; no device, no launch
static int plan_rows_here(NsqParams *p, int *grid, int occ, double recBytes, const PgKnobs &kn, int maxRows = PG_RB) {
  const int cus = cu_count();
  if (cus <= 0) return pg_fail(PG_E_NODEV, "no HIP device");
  set_rows_plan(p, grid, plan_rows(p->nrows, p->ncols, cus, occ, recBytes, kn, maxRows), kn);
  return 0;
}

extern "C" {

int pg_pack_planes(const void *src, int elem_bytes, int64_t n, int l, int64_t ld, const int64_t *rows, int bits,
                   void *planes, int64_t npad, uint32_t *flags, void *stream) {
  if (!src || !planes || !flags || n < 0 || ld < l) return pg_fail(PG_E_BADARG, "pg_pack_planes: bad argument");
  if (int rc = check_bits(bits)) return rc;
  if (int rc = check_l(l, bits, true)) return rc;
  if (npad < n || npad % 256) return pg_fail(PG_E_BADARG, "pg_pack_planes: npad must be pg_npad(n)");
  const int ng = pg_ngroups(l), nq = pg_nchunks(l, bits);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return pg_launched((int)e, "hipMemsetAsync");
  const dim3 grid((unsigned)(npad / PG_PACK_SEQS)), block(256);
  const long long *r = (const long long *)rows;
  u32 *pl = (u32 *)planes;
#define PG_PACK(T)                                                                                          \
  do {                                                                                                      \
    if (bits == 5) pg_pack_kernel<T, 5><<<grid, block, 0, s>>>((const T *)src, n, l, ld, r, pl, npad, ng, nq, flags); \
    else pg_pack_kernel<T, 8><<<grid, block, 0, s>>>((const T *)src, n, l, ld, r, pl, npad, ng, nq, flags); \
  } while (0)
  switch (elem_bytes) {
    case 1: PG_PACK(unsigned char); break;
    case 2: PG_PACK(short); break;
    case 4: PG_PACK(int); break;
    case 8: PG_PACK(long long); break;
    default: return pg_fail(PG_E_BADARG, "pg_pack_planes: elem_bytes must be 1, 2, 4 or 8");
  }
#undef PG_PACK
  return pg_launched("pg_pack_kernel");
}

int pg_pack_bytes(const uint8_t *src, int64_t n, int width, int64_t ld, const int64_t *rows, const uint8_t *lut256, int bits,
                  void *planes, int64_t npad, uint8_t *tokens_out, uint32_t *flags, void *stream) {
  if (!src || !lut256 || !planes || !flags || n < 0 || ld < width) return pg_fail(PG_E_BADARG, "pg_pack_bytes: bad argument");
  if (int rc = check_bits(bits)) return rc;
  if (int rc = check_l(width, bits, true)) return rc;
  if (npad < n || npad % 256) return pg_fail(PG_E_BADARG, "pg_pack_bytes: npad must be pg_npad(n)");
  const int ng = pg_ngroups(width), nq = pg_nchunks(width, bits);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return pg_launched((int)e, "hipMemsetAsync");
  const dim3 grid((unsigned)(npad / PG_PACK_SEQS)), block(256);
  if (bits == 5)
    pg_pack_kernel<unsigned char, 5><<<grid, block, 0, s>>>(src, n, width, ld, (const long long *)rows, (u32 *)planes, npad, ng, nq,
                                                            flags, lut256, tokens_out);
  else
    pg_pack_kernel<unsigned char, 8><<<grid, block, 0, s>>>(src, n, width, ld, (const long long *)rows, (u32 *)planes, npad, ng, nq,
                                                            flags, lut256, tokens_out);
  return pg_launched("pg_pack_kernel(bytes)");
}

int pg_hamming_dense(const void *x_planes, int64_t n, int64_t x_npad, const void *y_planes, int64_t m, int64_t y_npad,
                     int l, int bits, void *out, int out_elem_bytes, int64_t ldo, int accumulate, void *stream) {
  if (!x_planes || !y_planes || !out || n <= 0 || m <= 0 || ldo < n)
    return pg_fail(PG_E_BADARG, "pg_hamming_dense: bad argument");
  if (int rc = check_bits(bits)) return rc;
  if (int rc = check_l(l, bits)) return rc;
  if (out_elem_bytes != 1 && out_elem_bytes != 2 && out_elem_bytes != 4 && out_elem_bytes != 8)
    return pg_fail(PG_E_BADARG, "pg_hamming_dense: out_elem_bytes must be 1, 2, 4 or 8");
  if (x_npad < n || x_npad % 256 || y_npad < m) return pg_fail(PG_E_BADARG, "pg_hamming_dense: bad npad");
  if ((m + PG_RBD - 1) / PG_RBD > 65535) return pg_fail(PG_E_BADARG, "pg_hamming_dense: m too large for one launch");
  DenseParams p;
  p.xPlanes = (const uint4 *)x_planes; p.xNpad = x_npad; p.n = n;
  p.yPlanes = (const uint4 *)y_planes; p.yNpad = y_npad; p.m = m;
  p.out = out; p.ldo = ldo; p.outBytes = out_elem_bytes; p.accumulate = accumulate ? 1 : 0;
  return pg_launched(kDense[pg_ngroups(l) - 1](bits, p, (hipStream_t)stream), "pg_dense_kernel");
}

static int fill_nsq(NsqParams *p, const void *row_planes, int64_t row_npad, int64_t row0, int64_t nrows,
                    const void *col_planes, int64_t col_npad, int64_t ncols, int l, int bits, const PgKnobs &kn) {
  if (!row_planes || !col_planes || row0 < 0 || nrows <= 0 || ncols <= 0) return pg_fail(PG_E_BADARG, "bad argument");
  if (int rc = check_bits(bits)) return rc;
  if (int rc = check_l(l, bits)) return rc;
  if (col_npad < ncols || col_npad % 256 || row_npad < row0 + nrows) return pg_fail(PG_E_BADARG, "bad npad");
  if (ncols > 0x7fffffffLL) return pg_fail(PG_E_TOOMANY, "ncols exceeds int32 indices");
  memset(p, 0, sizeof(*p));
  p->filter = (int)kn.lbFilter.v;   // stage-1 lower-bound filter: adaptive by default; PG_LB_FILTER=0 disables, =2 forces it on
  p->rowPlanes = (const uint4 *)row_planes; p->rowNpad = row_npad; p->row0 = row0; p->nrows = nrows;
  p->colPlanes = (const uint4 *)col_planes; p->colNpad = col_npad; p->ncols = ncols;
  p->colSig = p->colPlanes + (long long)pg_nchunks(l, bits) * col_npad;
  p->colFold = p->colSig + 2 * col_npad;
  p->rowFold = p->rowPlanes + ((long long)pg_nchunks(l, bits) + 2) * row_npad;
  return 0;
}

#ifdef PG_MM_STATS
static unsigned long long *g_stats = nullptr;
extern "C" int pg_debug_stats(unsigned long long *out12, int reset) {   // debug builds only (tools/mm_stats.py); PG_NSTAT counters
  const size_t nst = PG_NSTAT + 2 * 65536;                 // the counters, then (start, duration) of the first 65536 passes
  if (!g_stats) { if (hipMalloc(&g_stats, nst * 8) != hipSuccess) return -1; hipMemset(g_stats, 0, nst * 8); }
  if (out12) { hipDeviceSynchronize(); hipMemcpy(out12, g_stats, (reset & 2 ? nst : PG_NSTAT) * 8, hipMemcpyDeviceToHost); }
  if (reset & 1) hipMemset(g_stats, 0, nst * 8);
  return 0;
}
#endif
typedef int (*mm_sym_fn)(const NsqParams &, int, hipStream_t);
static const mm_sym_fn kMmSym[8] = {pg_launch_mm_knn_sym_g1, pg_launch_mm_knn_sym_g2, pg_launch_mm_knn_sym_g3, pg_launch_mm_knn_sym_g4,
                                    pg_launch_mm_knn_sym_g5, pg_launch_mm_knn_sym_g6, pg_launch_mm_knn_sym_g7, pg_launch_mm_knn_sym_g8};
static const nsq_fn kMm[8] = {pg_launch_mm_g1, pg_launch_mm_g2, pg_launch_mm_g3, pg_launch_mm_g4,
                              pg_launch_mm_g5, pg_launch_mm_g6, pg_launch_mm_g7, pg_launch_mm_g8};
// resident workgroups per CU of an MFMA-engine instance (launcher mode codes 0..4), asked once from the runtime
static int mm_occupancy(int groups, int mode, int bits) {
  static std::atomic<int> cache[8][5][2];                  // (a property of the code object: the same on every gfx950)
  std::atomic<int> &c = cache[groups - 1][mode][bits == 8];
  int v = c.load(std::memory_order_relaxed);
  if (v == 0) {
    const int n = kMm[groups - 1](mode, bits, NsqParams(), -1, nullptr);
    v = n < 1 ? 4 : (n > 4 ? 4 : n);
    c.store(v, std::memory_order_relaxed);
  }
  return v;
}
// The pass plan of an MFMA-engine launch over `nrows` rows (plan_mm, pg_plan.h) goes into its parameters, with the
// engine's tuning knobs (*grid: its workgroups, where the caller has no plan of its own to read them from)
static void set_mm_plan(NsqParams *p, int *grid, int64_t nrows, const PassPlan &pl, const PgKnobs &kn) {
  p->rowsPerWave = pl.rowsPerWave; p->rowsPerPass = pl.rowsPerPass;
  p->mmTailFrom = pl.tailFrom; p->mmTailRows = pl.tailRows;
  if (kn.debugPlan.set) fprintf(stderr, "[pg plan mm] rows=%lld: %lld passes of %lld rows + %lld of %lld\n", (long long)nrows, pl.tailFrom, (long long)pl.rowsPerWave, pl.passes - pl.tailFrom, (long long)pl.tailRows);
  p->mmDenseL1 = (int)kn.mmL1.v;
  p->mmDenseL2 = (int)kn.mmL2.v;
  p->mmDirectRun = (int)kn.mmRun.v;
#ifdef PG_MM_STATS
  if (!g_stats) pg_debug_stats(nullptr, 1);
  p->stats = g_stats;
#endif
  p->mmPasses = pl.passes; p->mmGridWaves = pl.gridWaves;
  if (grid) *grid = pl.grid;
}
// The pass counter of a launch lives in the caller's workspace (pg_workspace_bytes): zeroed on the launch's stream
// right before the kernel.  Launch-private by contract, so concurrent launches - other streams, other devices,
// any number of them - never share a word (the static ring of counters this replaces did after 256 launches).
// Behind a probe (`probed`: run_probe on this workspace, this stream, in this call) pg_decide_kernel has zeroed the block.
static int pass_counter(NsqParams *p, void *workspace, hipStream_t s, bool probed = false) {
  if (!workspace) return pg_fail(PG_E_BADARG, "workspace required (pg_workspace_bytes)");
  unsigned *c = (unsigned *)workspace;
  if (!probed) {
    const hipError_t e = hipMemsetAsync(c, 0, PG_WS_GATES, s);   // (the counters and the row-block flags of a launch in column pieces)
    if (e != hipSuccess) return pg_launched((int)e, "workspace: hipMemsetAsync");
  }
  p->mmPassCounter = c;
  return 0;
}

int pg_eps_slots(const void *row_planes, int64_t row_npad, int64_t row0, int64_t nrows, const void *col_planes,
                 int64_t col_npad, int64_t ncols, int l, int bits, int cmp, double eps, int cap, int32_t *slot_idx,
                 uint8_t *slot_w, uint32_t *counts, void *workspace, void *stream) {
  NsqParams p;
  const PgKnobs kn = read_knobs();
  if (int rc = fill_nsq(&p, row_planes, row_npad, row0, nrows, col_planes, col_npad, ncols, l, bits, kn)) return rc;
  if (!slot_idx || !slot_w || !counts || cap < 0 || cmp < PG_CMP_LE || cmp > PG_CMP_GT)
    return pg_fail(PG_E_BADARG, "pg_eps_slots: bad argument");
  eps_interval(cmp, eps, &p.lo, &p.span);
  p.hi1 = (p.lo > 0xFFFFFF00u - 1u) ? 0u : p.lo + p.span + 1u;   // empty interval: nothing can match
  p.cap = (u32)cap; p.slotIdx = slot_idx; p.slotW = slot_w; p.counts = counts;
  int grid = 0;
  p.epsOrdered = kn.epsOrdered.v != 0;
  if (use_mm_engine(nrows, kn, l, false)) {
    set_mm_plan(&p, &grid, nrows, plan_mm(nrows, cu_count(), kn), kn);
    if (int rc = pass_counter(&p, workspace, (hipStream_t)stream)) return rc;
    return pg_launched(kMm[pg_ngroups(l) - 1](PG_MODE_EPS, bits, p, grid, (hipStream_t)stream), "pg_mm_kernel(eps)");
  }
  if (int rc = plan_rows_here(&p, &grid, nsq_occupancy(pg_ngroups(l), PG_MODE_EPS, bits), 16.0 * pg_nchunks(l, bits), kn)) return rc;
  return pg_launched(kNsq[pg_ngroups(l) - 1](PG_MODE_EPS, bits, p, grid, (hipStream_t)stream), "pg_nsq_kernel(eps)");
}

// Square self-graph, every unordered pair evaluated once (Hamming and the comparators are symmetric):
// the engine sweeps only columns above the row, a match (i, j) goes to the front of row i's slot
// in column order and to the back of row j's slot through an atomic counter.
int pg_eps_slots_sym(const void *planes, int64_t npad, int64_t n, int l, int bits, int cmp, double eps, int cap,
                     int32_t *slot_idx, uint8_t *slot_w, uint32_t *counts_up, uint32_t *counts_lo, void *workspace,
                     void *stream) {
  NsqParams p;
  const PgKnobs kn = read_knobs();
  if (int rc = fill_nsq(&p, planes, npad, 0, n, planes, npad, n, l, bits, kn)) return rc;
  if (!slot_idx || !slot_w || !counts_up || !counts_lo || cap < 0 || cmp < PG_CMP_LE || cmp > PG_CMP_GT)
    return pg_fail(PG_E_BADARG, "pg_eps_slots_sym: bad argument");
  if (n >= (1ll << 27)) return pg_fail(PG_E_TOOMANY, "pg_eps_slots_sym: n must be below 2^27");
  eps_interval(cmp, eps, &p.lo, &p.span);
  p.hi1 = (p.lo > 0xFFFFFF00u - 1u) ? 0u : p.lo + p.span + 1u;
  p.cap = (u32)cap; p.slotIdx = slot_idx; p.slotW = slot_w; p.counts = counts_up; p.countsLo = counts_lo;
  hipError_t e = hipMemsetAsync(counts_lo, 0, (size_t)n * sizeof(uint32_t), (hipStream_t)stream);
  if (e != hipSuccess) return pg_launched((int)e, "hipMemsetAsync");
  int grid = 0;
  // Large graphs: the data decide (probe above) between this path and a plain rectangular sweep on the VALU engine,
  // which writes the same slots (every match at the front of its row, counts_lo stays zero): dense graphs.
  if (probe_enabled(kn) && n >= PG_PROBE_MIN_N) {
    const u32 *gate = nullptr;
    if (int rc = run_probe(p, l, bits, 0u, p.lo, p.span, 1u, workspace, (hipStream_t)stream, kn, &gate)) return rc;
    NsqParams r = p;
    r.countsLo = nullptr;
    r.gate = gate + 1; r.gateMask = 1u << 1;
    int rgrid = 0;
    if (int rc = plan_rows_here(&r, &rgrid, nsq_occupancy(pg_ngroups(l), PG_MODE_EPS, bits), 16.0 * pg_nchunks(l, bits), kn)) return rc;
    if (int rc = pg_launched(kNsq[pg_ngroups(l) - 1](PG_MODE_EPS, bits, r, rgrid, (hipStream_t)stream), "pg_nsq_kernel(eps, gated)")) return rc;
    p.gate = gate + 1; p.gateMask = 1u << 0;
  }
  // Rows near the top sweep almost everything, rows near the bottom almost nothing; workgroups are
  // dispatched in row order, i.e. longest first, which balances by itself once there are a few
  // waves per resident slot.  Measured (tools/eps_sym_probe.py): 8 rows per wave at N = 50k, 16 at
  // N = 100k .. 200k (more rows: too few waves to balance; fewer: the per-wave column stream shows).
  p.epsOrdered = kn.epsOrdered.v != 0;
  if (use_mm_engine(n, kn, l, false)) {
    // the symmetric sweep's passes are not equal work (a pass sweeps the columns above its rows): about one and a half
    // rounds of passes balance best (tools/dbg/eps_plan.py: N = 50k 8 rows per pass 0.40 ms against 0.43 / 0.59 for 14 / 32;
    // N = 100k 16 rows 0.61 against 0.66 / 0.71 for 26 / 32; N = 200k 32 rows 1.12 against 1.62 for 16)
    long long rs = (n + 6399) / 6400;                       // (tools/dbg/sym_rows.py: N = 50k 8 rows 0.375 ms, 10 rows 0.40; 40k: 8; 70k: 12)
    rs = (rs + 1) / 2 * 2;
    rs = rs < 8 ? 8 : (rs > PG_MM_RB ? PG_MM_RB : rs);
    // (records of up to three chunks - four waves per SIMD; longer ones, N = 100k L = 128: 0.75 against 0.67 with the old rule)
    const bool fine = pg_nchunks(l, bits) <= 3 && kn.mmPlan.v != 2;
    set_mm_plan(&p, &grid, n, plan_mm(n, cu_count(), kn, PG_MM_RB, 4, false, fine ? (int)rs : 0), kn);
    if (int rc = pass_counter(&p, workspace, (hipStream_t)stream, p.gate != nullptr)) return rc;
    return pg_launched(kMm[pg_ngroups(l) - 1](PG_MODE_EPS_SYM, bits, p, grid, (hipStream_t)stream), "pg_mm_kernel(eps sym)");
  }
  if (!kn.rowsPerWave.set && !kn.wavesPerCu.set) {
    const long long r = n >= 80000 ? 16 : 8;
    p.rowsPerWave = (int)r; p.rowsPerPass = (int)r;
    grid = (int)(((n + r - 1) / r + PG_WG_WAVES - 1) / PG_WG_WAVES);
  } else if (int rc = plan_rows_here(&p, &grid, nsq_occupancy(pg_ngroups(l), PG_MODE_EPS_SYM, bits), 16.0 * pg_nchunks(l, bits), kn, 16)) {
    return rc;
  }
  return pg_launched(kNsq[pg_ngroups(l) - 1](PG_MODE_EPS_SYM, bits, p, grid, (hipStream_t)stream), "pg_nsq_kernel(eps sym)");
}

int pg_eps_compact_sym(const void *planes, int64_t npad, int64_t n, int l, int bits, int cmp, double eps, int cap,
                       const int32_t *slot_idx, const uint8_t *slot_w, const uint32_t *counts_up,
                       const uint32_t *counts_lo, const int64_t *indptr, int32_t *indices, uint8_t *weights,
                       int leave_overflow, void *stream) {
  CompactParams c;
  c.skipOverflow = leave_overflow ? 1 : 0;
  if (int rc = fill_nsq(&c.e, planes, npad, 0, n, planes, npad, n, l, bits, read_knobs())) return rc;
  if (!slot_idx || !slot_w || !counts_up || !counts_lo || !indptr || cap < 0 || cmp < PG_CMP_LE || cmp > PG_CMP_GT)
    return pg_fail(PG_E_BADARG, "pg_eps_compact_sym: bad argument");
  eps_interval(cmp, eps, &c.e.lo, &c.e.span);
  c.e.hi1 = c.e.lo + c.e.span + 1u;
  c.e.cap = (u32)cap;
  c.e.slotIdx = const_cast<int *>(slot_idx);
  c.e.slotW = const_cast<unsigned char *>(slot_w);
  c.e.counts = const_cast<u32 *>(counts_up);
  c.e.countsLo = const_cast<u32 *>(counts_lo);
  c.indptr = (const long long *)indptr; c.indices = indices; c.weights = weights;
  return pg_launched(kCompact[pg_ngroups(l) - 1](bits, c, (hipStream_t)stream), "pg_compact_kernel(sym)");
}

int64_t pg_scan_scratch_bytes(int64_t n) {
  const int64_t nb = (n + PG_SCAN_TILE - 1) / PG_SCAN_TILE;
  return (nb + 2) * (int64_t)sizeof(long long);
}

int pg_exclusive_scan(const uint32_t *counts, int64_t n, int64_t *indptr, void *scratch, void *stream) {
  if (!counts || !indptr || !scratch || n <= 0) return pg_fail(PG_E_BADARG, "pg_exclusive_scan: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const long long nb = (n + PG_SCAN_TILE - 1) / PG_SCAN_TILE;
  long long *part = (long long *)scratch;
  pg_scan_partials<u32><<<dim3((unsigned)nb), dim3(256), 0, s>>>(counts, n, part);
  pg_scan_single<<<dim3(1), dim3(256), 0, s>>>(part, nb);
  pg_scan_apply<u32, 0><<<dim3((unsigned)nb), dim3(256), 0, s>>>(counts, n, part, nb, (long long *)indptr, nullptr);
  return pg_launched("pg_scan");
}

int pg_eps_compact(const void *row_planes, int64_t row_npad, int64_t row0, int64_t nrows, const void *col_planes,
                   int64_t col_npad, int64_t ncols, int l, int bits, int cmp, double eps, int cap,
                   const int32_t *slot_idx, const uint8_t *slot_w, const uint32_t *counts, const int64_t *indptr,
                   int32_t *indices, uint8_t *weights, int leave_overflow, void *stream) {
  CompactParams c;
  c.skipOverflow = leave_overflow ? 1 : 0;
  if (int rc = fill_nsq(&c.e, row_planes, row_npad, row0, nrows, col_planes, col_npad, ncols, l, bits, read_knobs())) return rc;
  if (!slot_idx || !slot_w || !counts || !indptr || cap < 0 || cmp < PG_CMP_LE || cmp > PG_CMP_GT)
    return pg_fail(PG_E_BADARG, "pg_eps_compact: bad argument");
  eps_interval(cmp, eps, &c.e.lo, &c.e.span);
  c.e.hi1 = c.e.lo + c.e.span + 1u;
  c.e.cap = (u32)cap;
  c.e.slotIdx = const_cast<int *>(slot_idx);
  c.e.slotW = const_cast<unsigned char *>(slot_w);
  c.e.counts = const_cast<u32 *>(counts);
  c.indptr = (const long long *)indptr; c.indices = indices; c.weights = weights;
  return pg_launched(kCompact[pg_ngroups(l) - 1](bits, c, (hipStream_t)stream), "pg_compact_kernel");
}

// Rows whose matches did not fit their slot: the all-pairs engine runs once more over just those rows
// (row_list, relative to row0) and writes their matches, in column order, straight into the CSR at
// indptr[row] - exact for any slot capacity, at engine speed however many rows overflow.
int pg_eps_fill_rows(const void *row_planes, int64_t row_npad, int64_t row0, const int64_t *row_list, int64_t n_list,
                     const void *col_planes, int64_t col_npad, int64_t ncols, int l, int bits, int cmp, double eps,
                     const int64_t *indptr, int32_t *indices, uint8_t *weights, uint32_t *scratch_counts, void *workspace,
                     void *stream) {
  NsqParams p;
  if (!row_list || n_list <= 0) return pg_fail(PG_E_BADARG, "pg_eps_fill_rows: bad argument");
  const PgKnobs kn = read_knobs();
  if (int rc = fill_nsq(&p, row_planes, row_npad, row0, n_list, col_planes, col_npad, ncols, l, bits, kn)) return rc;
  if (!indptr || !indices || !weights || !scratch_counts || cmp < PG_CMP_LE || cmp > PG_CMP_GT)
    return pg_fail(PG_E_BADARG, "pg_eps_fill_rows: bad argument");
  eps_interval(cmp, eps, &p.lo, &p.span);
  p.hi1 = (p.lo > 0xFFFFFF00u - 1u) ? 0u : p.lo + p.span + 1u;
  p.cap = 0xFFFFFFFFu;                                     // a row's place in the CSR holds all of its matches
  p.rowList = (const long long *)row_list; p.fillIndptr = (const long long *)indptr;
  p.slotIdx = indices; p.slotW = weights; p.counts = scratch_counts;
  int grid = 0;
  set_mm_plan(&p, &grid, n_list, plan_mm(n_list, cu_count(), kn), kn);
  if (int rc = pass_counter(&p, workspace, (hipStream_t)stream)) return rc;
  return pg_launched(kMm[pg_ngroups(l) - 1](PG_MODE_EPS, bits, p, grid, (hipStream_t)stream), "pg_mm_kernel(eps fill)");
}

// ---------------------------------------------------------------------------------------
// A kNN launch: check, gather the hardware numbers, read the knobs, plan (knn_plan, pg_plan.h: every decision and the
// reasons), then run the plan's launches in order.  KnnRun is what the launches share; each launch_* below copies what
// its KnnPlan says into parameters and issues one launch - none of them decides anything.
// ---------------------------------------------------------------------------------------
struct KnnRun {
  const KnnPlan &pl;
  const PgKnobs &kn;
  NsqParams p;               // the main launch's parameters; the other launches start from a copy
  int l, bits, ng, k;
  int64_t row0, nrows;
  int32_t *idx;
  uint8_t *dist;
  void *workspace;
  hipStream_t stream;
  u32 *gates() const { return (u32 *)((char *)workspace + PG_WS_GATES); }
};
// resident workgroups per CU of the instances a launch of this shape may use
static KnnHw knn_hw(const KnnShape &s, const PgKnobs &kn) {
  const int ng = pg_ngroups(s.l);
  const bool shortList = knn_short_list(s, kn);
  KnnHw hw;
  hw.cus = cu_count();
  hw.occValu = nsq_occupancy(ng, PG_MODE_KNN, s.bits);
  hw.occMm32 = mm_occupancy(ng, shortList ? PG_MODE_KNN_SHORT : PG_MODE_KNN, s.bits);
  hw.occMm64 = shortList ? mm_occupancy(ng, PG_MODE_KNN_SHORT2, s.bits) : 0;
  static std::atomic<int> occCache[8];
  int occS = occCache[ng - 1].load(std::memory_order_relaxed);
  if (occS == 0) {
    const int n = kMmSym[ng - 1](NsqParams(), -1, nullptr);
    occS = n < 1 ? 4 : (n > 4 ? 4 : n);
    occCache[ng - 1].store(occS, std::memory_order_relaxed);
  }
  hw.occSym = occS;
  return hw;
}
// the VALU engine: the whole launch, or the alternative behind a probe (gated on gate[0] bit 1)
static int launch_valu(const KnnRun &r, bool gated) {
  NsqParams q = r.p;
  if (gated) { q.knnGuess = r.pl.guessValu; q.gate = r.gates(); q.gateMask = 1u << 1; }
  if (r.pl.valu.grid <= 0) return pg_fail(PG_E_NODEV, "no HIP device");   // (knn_plan plans no VALU launch for a device of no CUs)
  int grid = 0;
  set_rows_plan(&q, &grid, r.pl.valu, r.kn);
  return pg_launched(kNsq[r.ng - 1](PG_MODE_KNN, r.bits, q, grid, r.stream), "pg_nsq_kernel(knn)");
}
// the arguments of the sweep's plan, for its own launch or the probe's decision launch
static SymPlanArgs sym_plan_args(const KnnPlan &pl, void *workspace) {
  char *base = (char *)workspace + pl.symBase;
  return SymPlanArgs{pl.symNb, pl.symNst, pl.symSlots, pl.symPiece, pl.symPieceMin, (int4 *)(base + pl.symWs.plan), (u32 *)(base + pl.symWs.pieceStart),
                     (uint4 *)(base + pl.symWs.lowCount), pl.symZero4, pl.symPlanGrid};
}
// the symmetric sweep of a self graph, in front of the rectangular launch: its plan kernel (where the plan did not ride in
// the probe's decision launch), the sweep, its merge
static int launch_sym(const KnnRun &r) {
  const KnnPlan &pl = r.pl;
  char *base = (char *)r.workspace + pl.symBase;
  NsqParams s = r.p;
  s.nrows = r.nrows;
  s.gateMask = pl.symGateMask;
  SymArgs sa;
  sa.plan = (const int4 *)(base + pl.symWs.plan); sa.partial = (u32 *)(base + pl.symWs.partial);
  sa.lowCount = (u32 *)(base + pl.symWs.lowCount); sa.lowKeys = (u32 *)(base + pl.symWs.lowKeys);
  sa.capL = pl.symCapL;
  sa.deliver = pl.symDeliver;
  sa.rowBits = pl.symRowBits;
  pg_sym_set(&s, sa);
  s.mmEvict = nullptr; s.mmEvictRows = nullptr; s.mmPieces = 0; s.mmPieceFrom = 0; s.mmPartial = nullptr;
  s.rowsPerWave = 2 * PG_MM_RB; s.rowsPerPass = 2 * PG_MM_RB; s.mmTailFrom = pl.symPasses; s.mmTailRows = 2 * PG_MM_RB;
  s.mmPasses = pl.symPasses;
  s.mmGridWaves = pl.symGridWaves;
  s.mmPassCounter = r.p.mmPassCounter + 16;
  u32 *pieceStart = (u32 *)(base + pl.symWs.pieceStart), *gate2 = r.gates() + 2;
  if (r.kn.debugPlan.set) fprintf(stderr, "[pg plan sym] rows=%lld: %lld passes for %lld slots, plan %s, merge window %d\n", (long long)r.nrows, pl.symPasses, pl.symSlots,
                                 pl.symPlanRides ? "rides in the decide launch" : "launched", pl.symMergeWindow);
  if (!pl.symPlanRides) {
    pg_knn_sym_plan_kernel<<<dim3(pl.symPlanGrid), dim3(1024), 0, r.stream>>>(sym_plan_args(pl, r.workspace));
    if (int rc = pg_launched("pg_knn_sym_plan_kernel")) return rc;
  }
  if (int rc = pg_launched(kMmSym[r.ng - 1](s, (int)(s.mmGridWaves / PG_WG_WAVES), r.stream), "pg_mm_knn_sym_kernel")) return rc;
  auto *merge = pl.symMergeWindow == 1 ? pg_knn_sym_merge_kernel<1> : (pl.symMergeWindow == 2 ? pg_knn_sym_merge_kernel<2> : pg_knn_sym_merge_kernel<4>);
  merge<<<dim3(pl.symMergeGrid), dim3(PG_WG_THREADS), 0, r.stream>>>(
      sa.partial, pieceStart, sa.lowCount, sa.lowKeys, sa.capL, sa.rowBits, r.nrows, r.k, r.idx, r.dist, r.p.knnGuess, r.p.mmEvict,
      r.p.mmEvictRows, s.gate, s.gateMask, gate2, r.p.mmPassCounter + 17, (u32)(pl.symLimit < 0 ? 0 : pl.symLimit));
  return pg_launched("pg_knn_sym_merge_kernel");
}
// the main launch of the MFMA engine (r.p: the plain passes, the gate and the eviction are set), with the column pieces
// of the rows beyond mainRows and their merge when the plan splits
static int launch_main(KnnRun &r) {
  const KnnPlan &pl = r.pl;
  NsqParams &p = r.p;
  if (!pl.split) return pg_launched(kMm[r.ng - 1](pl.mode, r.bits, p, pl.launch.grid, r.stream), "pg_mm_kernel(knn)");
  const long long rem = r.nrows - pl.mainRows;
  p.nrows = r.nrows;
  p.mmPieces = pl.pieces; p.mmPieceFrom = pl.main.passes; p.mmPartial = (u32 *)((char *)r.workspace + PG_WS_PARTIAL);
  p.mmPasses = pl.launch.passes;
  p.mmTailFrom = pl.launch.tailFrom; p.mmTailRows = pl.launch.tailRows;
  p.mmGridWaves = pl.launch.gridWaves;
  if (int rc = pg_launched(kMm[r.ng - 1](pl.mode, r.bits, p, pl.launch.grid, r.stream), "pg_mm_kernel(knn + column pieces)")) return rc;
  pg_knn_merge_kernel<<<dim3(pl.pieceMergeGrid), dim3(PG_WG_THREADS), 0, r.stream>>>(
      p.mmPartial, rem, pl.pieces, r.k, r.idx + pl.mainRows * r.k, r.dist + pl.mainRows * r.k, p.knnGuess, p.mmEvict, p.mmEvictRows,
      (long long)r.row0 + pl.mainRows, p.gate, p.gateMask);
  return pg_launched("pg_knn_merge_kernel");
}
// the probe may say "one cluster" (gate 2): the same engine with 32-row passes over all rows, as a third alternative
static int launch_alt32(const KnnRun &r) {
  NsqParams q = r.p;
  q.nrows = r.nrows;
  q.mmPieces = 0; q.mmPieceFrom = 0; q.mmPartial = nullptr;
  q.mmEvict = nullptr; q.mmEvictRows = nullptr;             // (one cluster: every row has its neighbours; the second phase if not)
  set_mm_plan(&q, nullptr, r.nrows, r.pl.alt, r.kn);
  q.mmPassCounter = r.p.mmPassCounter + 8;
  q.gateMask = 1u << 2;
  return pg_launched(kMm[r.ng - 1](PG_MODE_KNN_SHORT, r.bits, q, r.pl.alt.grid, r.stream), "pg_mm_kernel(knn, 32-row passes, gated)");
}
// the evicted rows, behind everything else: one exact sweep of all columns per row
static int launch_evicted(const KnnRun &r) {
  const NsqParams &p = r.p;
  KnnRowsParams kr;
  kr.rowPlanes = p.rowPlanes; kr.colPlanes = p.colPlanes; kr.rowNpad = p.rowNpad; kr.colNpad = p.colNpad; kr.ncols = p.ncols;
  kr.count = p.mmEvict; kr.rows = p.mmEvictRows; kr.baseRow = r.row0; kr.k = r.k;
  kr.knnIdx = r.idx; kr.knnDist = r.dist; kr.gate = p.gate; kr.gateMask = r.pl.evictGateMask;
  return pg_launched(kKnnRows[r.ng - 1](r.bits, kr, r.pl.evictGrid, r.stream), "pg_knn_rows_kernel");
}

static int knn_launch(const void *row_planes, int64_t row_npad, int64_t row0, int64_t nrows, const void *col_planes,
                      int64_t col_npad, int64_t ncols, int l, int bits, int k, int first, const uint32_t *floor_keys,
                      uint32_t *last_keys, int32_t *idx_out, uint8_t *dist_out, void *workspace, void *stream) {
  const PgKnobs kn = read_knobs();
  NsqParams p;
  if (int rc = fill_nsq(&p, row_planes, row_npad, row0, nrows, col_planes, col_npad, ncols, l, bits, kn)) return rc;
  if (!idx_out || !dist_out) return pg_fail(PG_E_BADARG, "pg_knn_hamming: bad argument");
  if (k < 1 || first < 0 || first > 1 || first + k > 64) return pg_fail(PG_E_BADARG, "pg_knn_hamming: k out of range");
  if (ncols > PG_MAX_N_KNN) return pg_fail(PG_E_TOOMANY, "pg_knn_hamming: ncols exceeds 2^24");
  KnnShape shape;
  shape.nrows = nrows; shape.ncols = ncols; shape.row0 = row0;
  shape.samePlanes = row_planes == col_planes && row_npad == col_npad;
  shape.l = l; shape.bits = bits; shape.k = k; shape.first = first;
  shape.floorKeys = floor_keys != nullptr; shape.lastKeys = last_keys != nullptr; shape.workspace = workspace != nullptr;
  const KnnPlan pl = knn_plan(shape, knn_hw(shape, kn), kn);

  p.k = k; p.knnFirst = first; p.floorKeys = floor_keys; p.lastKeys = last_keys;
  p.knnGuess = pl.guess;
  p.knnIdx = idx_out; p.knnDist = dist_out;
  KnnRun r = {pl, kn, p, l, bits, pg_ngroups(l), k, row0, nrows, idx_out, dist_out, workspace, (hipStream_t)stream};
  if (!pl.mm) return launch_valu(r, false);
  if (pl.probe) {
    const u32 *gate = nullptr;
    const SymPlanArgs ride = pl.symPlanRides ? sym_plan_args(pl, workspace) : SymPlanArgs{};
    if (int rc = run_probe(r.p, l, bits, pl.guess, 1u, 0u, (u32)(first + k), workspace, r.stream, kn, &gate, pl.symPlanRides ? &ride : nullptr)) return rc;
    if (int rc = launch_valu(r, true)) return rc;
    r.p.gate = gate;
  }
  r.p.gateMask = pl.mainGateMask;
  set_mm_plan(&r.p, nullptr, pl.mainRows, pl.main, kn);
  r.p.nrows = pl.mainRows;
  if (int rc = pass_counter(&r.p, workspace, r.stream, pl.probe)) return rc;
  if (pl.evict) {
    r.p.mmEvict = (u32 *)workspace + 1;                     // (word 1 of the counter line: zeroed by pass_counter)
    r.p.mmEvictRows = (u32 *)((char *)workspace + pl.evictOffset);
  }
  if (pl.sym) {
    if (int rc = launch_sym(r)) return rc;
    r.p.gate = r.gates() + 2;
  }
  if (pl.split) {                                           // (the main launch and the pieces go out before the alternative)
    if (int rc = launch_main(r)) return rc;
  }
  if (pl.alt32) {
    if (int rc = launch_alt32(r)) return rc;
  }
  if (!pl.split) {
    if (int rc = launch_main(r)) return rc;
  }
  return pl.evict ? launch_evicted(r) : 0;
}

int pg_knn_hamming(const void *row_planes, int64_t row_npad, int64_t row0, int64_t nrows, const void *col_planes,
                   int64_t col_npad, int64_t ncols, int l, int bits, int k, int32_t *idx_out, uint8_t *dist_out,
                   void *workspace, void *stream) {
  if (k < 1 || k > PG_MAX_K) return pg_fail(PG_E_BADARG, "pg_knn_hamming: k must be in 1..63");
  return knn_launch(row_planes, row_npad, row0, nrows, col_planes, col_npad, ncols, l, bits, k, 1, nullptr, nullptr,
                    idx_out, dist_out, workspace, stream);
}

int pg_knn_hamming_round(const void *row_planes, int64_t row_npad, int64_t row0, int64_t nrows, const void *col_planes,
                         int64_t col_npad, int64_t ncols, int l, int bits, int k, int first_round,
                         const uint32_t *floor_keys, uint32_t *last_keys, int32_t *idx_out, uint8_t *dist_out,
                         void *workspace, void *stream) {
  if (!last_keys || (!first_round && !floor_keys)) return pg_fail(PG_E_BADARG, "pg_knn_hamming_round: key arrays required");
  return knn_launch(row_planes, row_npad, row0, nrows, col_planes, col_npad, ncols, l, bits, k, first_round ? 1 : 0,
                    first_round ? nullptr : floor_keys, last_keys, idx_out, dist_out, workspace, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// Queries against a database (pg_query_knn_hamming).  Pieces per query group: enough workgroups to give every CU about
// eight (a single query against 200 000 sequences: 391 tiles of 128 columns -> about a hundred pieces), at least four
// tiles per piece (one per wave), and pieces x k within what the merge kernel holds in LDS.  A function of (nq, ndb, k)
// only, so that pg_query_workspace_bytes and the call agree; the call then bounds it by the workspace it was given.
// ---------------------------------------------------------------------------------------
#define PG_QUERY_TARGET_WG 2048
static int query_pieces(int64_t nq, int64_t ndb, int k) {
  const long long ngrp = (nq + PG_QUERY_RW - 1) / PG_QUERY_RW;
  const long long ntiles = (ndb + PG_QUERY_TILE - 1) / PG_QUERY_TILE;
  long long p = (PG_QUERY_TARGET_WG + ngrp - 1) / ngrp;
  const long long byTiles = (ntiles + 3) / 4, byLds = PG_QUERY_MERGE_KEYS / (k > 0 ? k : 1);
  if (p > byTiles) p = byTiles;
  if (p > byLds) p = byLds;
  return (int)(p < 1 ? 1 : p);
}

// one workgroup per query: its pieces x k keys (sorted lists of k) into LDS with independent loads, the four waves each
// insert a quarter of them into a 64-lane list (pg_query_knn_kernel's insertion), the four lists merged as there
__global__ __launch_bounds__(PG_WG_THREADS) void pg_query_merge_kernel(const u32 *partial, int pieces, int k, int *idx,
                                                                       unsigned char *dist, u32 *lastKeys) {
  __shared__ u32 keys[PG_QUERY_MERGE_KEYS];
  __shared__ u32 lists[PG_WG_WAVES][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long q = blockIdx.x;
  const int n = pieces * k;
  const u32 *src = partial + q * (long long)n;
  for (int e = threadIdx.x; e < n; e += PG_WG_THREADS) keys[e] = src[e];
  __syncthreads();
  u32 l = 0xFFFFFFFFu, t = 0xFFFFFFFFu;
  for (int e0 = wv * 64; e0 < n; e0 += PG_WG_WAVES * 64) {
    const u32 key = e0 + lane < n ? keys[e0 + lane] : 0xFFFFFFFFu;
    u64 m = __builtin_amdgcn_ballot_w64(key < t);
    while (m) {
      const int j = __builtin_ctzll(m);
      m &= m - 1;
      const u32 x = (u32)__builtin_amdgcn_readlane((int)key, j);
      if (x < t) {
        const u32 prev = wave_shr1(l, 0u);
        l = (l <= x) ? l : (prev > x ? prev : x);
        t = (u32)__builtin_amdgcn_readlane((int)l, k - 1);
      }
    }
  }
  lists[wv][lane] = l;
  __syncthreads();
  if (wv != 0) return;
  for (int w = 1; w < PG_WG_WAVES; ++w) {
    const u32 other = lists[w][lane];
    u64 m = __builtin_amdgcn_ballot_w64(other < t && lane < k);
    while (m) {
      const int j = __builtin_ctzll(m);
      m &= m - 1;
      const u32 x = (u32)__builtin_amdgcn_readlane((int)other, j);
      if (x < t) {
        const u32 prev = wave_shr1(l, 0u);
        l = (l <= x) ? l : (prev > x ? prev : x);
        t = (u32)__builtin_amdgcn_readlane((int)l, k - 1);
      }
    }
  }
  if (lane < k) {
    idx[q * k + lane] = l == 0xFFFFFFFFu ? -1 : (int)(l & 0x00FFFFFFu);
    dist[q * k + lane] = (unsigned char)(l >> 24);
    if (lastKeys && lane == k - 1) lastKeys[q] = l;
  }
}

typedef int (*query_fn)(int, const QueryParams &, long long, hipStream_t);
static const query_fn kQuery[8] = {pg_launch_query_g1, pg_launch_query_g2, pg_launch_query_g3, pg_launch_query_g4,
                                   pg_launch_query_g5, pg_launch_query_g6, pg_launch_query_g7, pg_launch_query_g8};

extern "C" {

int64_t pg_query_workspace_bytes(int64_t nq, int64_t ndb, int k) {
  if (nq <= 0 || ndb <= 0 || k < 1 || k > 64) return 0;
  const int pieces = query_pieces(nq, ndb, k);
  return pieces > 1 ? (int64_t)nq * pieces * k * 4 : 0;
}

int pg_query_knn_hamming(const void *q_planes, int64_t nq, int64_t q_npad, const void *db_planes, int64_t ndb,
                         int64_t db_npad, int l, int bits, int k, const uint32_t *floor_keys, uint32_t *last_keys,
                         int32_t *idx_out, uint8_t *dist_out, void *workspace, int64_t workspace_bytes, void *stream) {
  if (!q_planes || !db_planes || !idx_out || !dist_out || nq <= 0 || ndb <= 0 || workspace_bytes < 0)
    return pg_fail(PG_E_BADARG, "pg_query_knn_hamming: bad argument");
  if (k < 1 || k > 64) return pg_fail(PG_E_BADARG, "pg_query_knn_hamming: k must be in 1..64");
  if (int rc = check_bits(bits)) return rc;
  if (int rc = check_l(l, bits)) return rc;
  if (q_npad < nq || db_npad < ndb || db_npad % 256) return pg_fail(PG_E_BADARG, "pg_query_knn_hamming: bad npad");
  if (ndb >= PG_MAX_N_KNN) return pg_fail(PG_E_TOOMANY, "pg_query_knn_hamming: ndb must be below 2^24");
  // pieces: the plan, bounded by the workspace the caller passed (pg_query_workspace_bytes gives the plan's size)
  long long pieces = query_pieces(nq, ndb, k);
  const long long fit = workspace ? workspace_bytes / ((long long)nq * k * 4) : 0;
  if (pieces > fit) pieces = fit < 1 ? 1 : fit;
  if (pieces > PG_QUERY_MERGE_KEYS / k) pieces = PG_QUERY_MERGE_KEYS / k;
  QueryParams p;
  p.qPlanes = (const uint4 *)q_planes; p.dbPlanes = (const uint4 *)db_planes;
  p.qNpad = q_npad; p.dbNpad = db_npad; p.nq = nq; p.ndb = ndb;
  p.k = k; p.pieces = (int)pieces;
  const long long ntiles = (ndb + PG_QUERY_TILE - 1) / PG_QUERY_TILE;
  p.tilesPerPiece = (ntiles + pieces - 1) / pieces;
  p.pieces = (int)((ntiles + p.tilesPerPiece - 1) / p.tilesPerPiece);   // (no empty piece)
  p.floorKeys = floor_keys; p.partial = (u32 *)workspace;
  p.knnIdx = idx_out; p.knnDist = dist_out; p.lastKeys = last_keys;
  const long long ngrp = (nq + PG_QUERY_RW - 1) / PG_QUERY_RW;
  if (ngrp * p.pieces > 0x7FFFFFFFll) return pg_fail(PG_E_TOOMANY, "pg_query_knn_hamming: too many queries for one launch");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = pg_launched(kQuery[pg_ngroups(l) - 1](bits, p, ngrp * p.pieces, s), "pg_query_knn_kernel")) return rc;
  if (p.pieces == 1) return 0;
  if (nq > 0x7FFFFFFFll) return pg_fail(PG_E_TOOMANY, "pg_query_knn_hamming: too many queries for one launch");
  pg_query_merge_kernel<<<dim3((unsigned)nq), dim3(PG_WG_THREADS), 0, s>>>((const u32 *)workspace, p.pieces, k, idx_out,
                                                                             dist_out, last_keys);
  return pg_launched("pg_query_merge_kernel");
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// eps rows of queries (pg_query_eps_count / _fill): the piece plan of pg_query_knn_hamming without the merge kernel's LDS
// bound.  A function of (nq, ndb) only; the caller sizes the segment tables from it (pg_query_eps_segments) and passes
// the segment count back, so count and fill sweep the same segments.
// ---------------------------------------------------------------------------------------
static long long query_eps_pieces(int64_t nq, int64_t ndb) {
  const long long ngrp = (nq + PG_QUERY_RW - 1) / PG_QUERY_RW;
  const long long ntiles = (ndb + PG_QUERY_TILE - 1) / PG_QUERY_TILE;
  long long p = (PG_QUERY_TARGET_WG + ngrp - 1) / ngrp;
  const long long byTiles = (ntiles + PG_WG_WAVES - 1) / PG_WG_WAVES;   // at least one tile per wave
  if (p > byTiles) p = byTiles;
  return p < 1 ? 1 : p;
}

typedef int (*query_eps_fn)(int, int, const QueryEpsParams &, long long, hipStream_t);
static const query_eps_fn kQueryEps[8] = {pg_launch_query_eps_g1, pg_launch_query_eps_g2, pg_launch_query_eps_g3,
                                          pg_launch_query_eps_g4, pg_launch_query_eps_g5, pg_launch_query_eps_g6,
                                          pg_launch_query_eps_g7, pg_launch_query_eps_g8};

// the checks and the launch both entries share; every check runs on the host before the launch
static int query_eps_launch(const char *who, int fill, const void *q_planes, int64_t nq, int64_t q_npad,
                            const void *db_planes, int64_t ndb, int64_t db_npad, int l, int bits, int cmp, double eps,
                            int64_t nseg, QueryEpsParams &p, void *stream) {
  if (!q_planes || !db_planes || nq <= 0 || ndb <= 0 || cmp < PG_CMP_LE || cmp > PG_CMP_GT || !(eps == eps))
    return pg_fail(PG_E_BADARG, who);
  if (int rc = check_bits(bits)) return rc;
  if (int rc = check_l(l, bits)) return rc;
  if (q_npad < nq || db_npad < ndb || db_npad % 256) return pg_fail(PG_E_BADARG, "pg_query_eps: bad npad");
  if (ndb > 0x7FFFFFFFll) return pg_fail(PG_E_TOOMANY, "pg_query_eps: ndb must fit int32 column indices");
  const long long ntiles = (ndb + PG_QUERY_TILE - 1) / PG_QUERY_TILE;
  if (nseg < PG_WG_WAVES || nseg % PG_WG_WAVES || nseg / PG_WG_WAVES > ntiles)
    return pg_fail(PG_E_BADARG, "pg_query_eps: nseg must be 4 x pieces, with at most one piece per column tile");
  const long long ngrp = (nq + PG_QUERY_RW - 1) / PG_QUERY_RW;
  const long long pieces = nseg / PG_WG_WAVES;
  if (ngrp * pieces > 0x7FFFFFFFll) return pg_fail(PG_E_TOOMANY, "pg_query_eps: too many queries for one launch");
  p.qPlanes = (const uint4 *)q_planes; p.dbPlanes = (const uint4 *)db_planes;
  p.qNpad = q_npad; p.dbNpad = db_npad; p.nq = nq; p.ndb = ndb;
  eps_interval(cmp, eps, &p.lo, &p.span, 0);
  p.pieces = (int)pieces;
  p.tilesPerPiece = (ntiles + pieces - 1) / pieces;        // (trailing pieces may be empty: their segments count 0)
  return pg_launched(kQueryEps[pg_ngroups(l) - 1](bits, fill, p, ngrp * pieces, (hipStream_t)stream),
                  fill ? "pg_query_eps_kernel(fill)" : "pg_query_eps_kernel(count)");
}

extern "C" {

int64_t pg_query_eps_segments(int64_t nq, int64_t ndb) {
  if (nq <= 0 || ndb <= 0) return 0;
  return query_eps_pieces(nq, ndb) * PG_WG_WAVES;
}

int pg_query_eps_count(const void *q_planes, int64_t nq, int64_t q_npad, const void *db_planes, int64_t ndb, int64_t db_npad,
                       int l, int bits, int cmp, double eps, int64_t nseg, uint32_t *seg_counts, void *stream) {
  if (!seg_counts) return pg_fail(PG_E_BADARG, "pg_query_eps_count: bad argument");
  QueryEpsParams p = {};
  p.segCounts = seg_counts;
  return query_eps_launch("pg_query_eps_count: bad argument", 0, q_planes, nq, q_npad, db_planes, ndb, db_npad, l, bits, cmp,
                          eps, nseg, p, stream);
}

int pg_query_eps_fill(const void *q_planes, int64_t nq, int64_t q_npad, const void *db_planes, int64_t ndb, int64_t db_npad,
                      int l, int bits, int cmp, double eps, int64_t nseg, const int64_t *seg_indptr, int32_t *indices,
                      uint8_t *weights, void *stream) {
  if (!seg_indptr || !indices || !weights) return pg_fail(PG_E_BADARG, "pg_query_eps_fill: bad argument");
  QueryEpsParams p = {};
  p.segIndptr = (const long long *)seg_indptr; p.indices = indices; p.weights = weights;
  return query_eps_launch("pg_query_eps_fill: bad argument", 1, q_planes, nq, q_npad, db_planes, ndb, db_npad, l, bits, cmp,
                          eps, nseg, p, stream);
}

int pg_index_flags(const void *planes, int64_t n, int64_t npad, int l, int bits, int64_t ref,
                   const uint32_t *want_dist, int pos_mode, const uint32_t *pos_mask, const uint32_t *not_mask,
                   uint8_t *dist_out, uint64_t *hist, uint8_t *flags, void *stream) {
  if (!planes || n <= 0 || npad < n || ref < 0 || ref >= n) return pg_fail(PG_E_BADARG, "pg_index_flags: bad argument");
  if (int rc = check_bits(bits)) return rc;
  if (int rc = check_l(l, bits, true)) return rc;         // the positions, not the padded width: 256 is beyond 5 bit planes
  if (pos_mode < 0 || pos_mode > 2 || (pos_mode && (!pos_mask || !not_mask)))
    return pg_fail(PG_E_BADARG, "pg_index_flags: bad position mode / masks");
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (bits == 5)
    pg_index_kernel<5><<<grid, block, 0, s>>>((const u32 *)planes, n, npad, pg_ngroups(l), ref, want_dist, pos_mode,
                                              pos_mask, not_mask, dist_out, (u64 *)hist, flags);
  else
    pg_index_kernel<8><<<grid, block, 0, s>>>((const u32 *)planes, n, npad, pg_ngroups(l), ref, want_dist, pos_mode,
                                              pos_mask, not_mask, dist_out, (u64 *)hist, flags);
  return pg_launched("pg_index_kernel");
}

// ---------------------------------------------------------------------------------------
// banded Levenshtein kNN (build defined; see pg_lev.hip)
// ---------------------------------------------------------------------------------------
int pg_lev_profile(const uint8_t *tokens, int64_t n, int l, int64_t ld, void *profiles, int64_t npad, int32_t *lens,
                   uint32_t *flags, void *stream) {
  if (!tokens || !profiles || !lens || !flags || n <= 0 || ld < l) return pg_fail(PG_E_BADARG, "pg_lev_profile: bad argument");
  if (int rc = check_l(l)) return rc;
  if (npad < n || npad % 256) return pg_fail(PG_E_BADARG, "pg_lev_profile: npad must be pg_npad(n)");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(flags, 0, sizeof(uint32_t), s);
  if (e != hipSuccess) return pg_launched((int)e, "hipMemsetAsync");
  return pg_launched(pg_launch_lev_profile(tokens, n, l, ld, (u32 *)profiles, npad, lens, flags, s), "pg_lev_profile_kernel");
}

int pg_lev_candidates(const void *profiles, int64_t npad, int64_t n, int64_t row0, int64_t nrows, int band, int cap,
                      int32_t *slot_idx, uint8_t *slot_w, uint32_t *counts, void *stream) {
  if (!profiles || !slot_idx || !slot_w || !counts || n <= 0 || nrows <= 0 || row0 < 0 || row0 + nrows > n || cap < 0)
    return pg_fail(PG_E_BADARG, "pg_lev_candidates: bad argument");
  if (band < 0 || band > PG_LEV_MAX_BAND) return pg_fail(PG_E_BADARG, "pg_lev_candidates: band must be in 0..8");
  if (npad < n || npad % 256) return pg_fail(PG_E_BADARG, "pg_lev_candidates: bad npad");
  if (n > 0x7fffffffLL) return pg_fail(PG_E_TOOMANY, "n exceeds int32 indices");
  NsqParams p;
  const PgKnobs kn = read_knobs();
  memset(&p, 0, sizeof(p));
  p.rowPlanes = (const uint4 *)profiles; p.rowNpad = npad; p.row0 = row0; p.nrows = nrows;
  p.colPlanes = (const uint4 *)profiles; p.colNpad = npad; p.ncols = n;
  p.lo = 0; p.span = 2u * (u32)band; p.hi1 = p.span + 1u;
  p.filter = (int)kn.lbFilter.v;             // keep pairs with max(SAD, 2*|dlen|) <= 2*band, self included
  p.cap = (u32)cap; p.slotIdx = slot_idx; p.slotW = slot_w; p.counts = counts;
  int grid = 0;
  static int bag_occ = 0;
  if (!bag_occ) { bag_occ = pg_occ_nsq_bag(); if (bag_occ < 1) bag_occ = 4; }
  if (int rc = plan_rows_here(&p, &grid, bag_occ, 48.0, kn)) return rc;
  return pg_launched(pg_launch_nsq_bag(p, grid, (hipStream_t)stream), "pg_nsq_kernel(bag)");
}

// Symmetric candidate generation (all rows against the same profiles): every unordered pair once,
// the row itself excluded; slots as in pg_eps_slots_sym.  pg_lev_knn takes both counters.
int pg_lev_candidates_sym(const void *profiles, int64_t npad, int64_t n, int band, int cap, int32_t *slot_idx,
                          uint8_t *slot_w, int32_t *slot_aux, uint32_t *counts_up, uint32_t *counts_lo, void *stream) {
  if (!profiles || !slot_idx || !slot_w || !counts_up || !counts_lo || n <= 0 || cap < 0)
    return pg_fail(PG_E_BADARG, "pg_lev_candidates_sym: bad argument");
  if (band < 0 || band > PG_LEV_MAX_BAND) return pg_fail(PG_E_BADARG, "pg_lev_candidates_sym: band must be in 0..8");
  if (npad < n || npad % 256) return pg_fail(PG_E_BADARG, "pg_lev_candidates_sym: bad npad");
  if (n >= (1ll << 27)) return pg_fail(PG_E_TOOMANY, "pg_lev_candidates_sym: n must be below 2^27");
  NsqParams p;
  const PgKnobs kn = read_knobs();
  memset(&p, 0, sizeof(p));
  p.rowPlanes = (const uint4 *)profiles; p.rowNpad = npad; p.row0 = 0; p.nrows = n;
  p.colPlanes = (const uint4 *)profiles; p.colNpad = npad; p.ncols = n;
  p.lo = 0; p.span = 2u * (u32)band; p.hi1 = p.span + 1u;
  p.filter = (int)kn.lbFilter.v;
  p.cap = (u32)cap; p.slotIdx = slot_idx; p.slotW = slot_w; p.slotAux = slot_aux; p.counts = counts_up; p.countsLo = counts_lo;
  hipError_t e = hipMemsetAsync(counts_lo, 0, (size_t)n * sizeof(uint32_t), (hipStream_t)stream);
  if (e != hipSuccess) return pg_launched((int)e, "hipMemsetAsync");
  long long r = n >= 80000 ? 16 : 8;                        // as pg_eps_slots_sym
  if (kn.rowsPerWave.v > 0) r = kn.rowsPerWave.v;
  p.rowsPerWave = (int)r; p.rowsPerPass = (int)(r > PG_RB ? PG_RB : r);
  const int grid = (int)(((n + r - 1) / r + PG_WG_WAVES - 1) / PG_WG_WAVES);
  return pg_launched(pg_launch_nsq_bag_sym(p, grid, (hipStream_t)stream), "pg_nsq_kernel(bag sym)");
}

int pg_lev_knn(const uint8_t *tokens, int64_t n, int l, int64_t ld, const void *planes128, int64_t npad,
               const int32_t *lens, int64_t row0, int64_t nrows,
               int band, int k, int cap, const int32_t *slot_idx, uint8_t *slot_w, const int32_t *slot_aux,
               const uint32_t *counts, const uint32_t *counts_lo, int32_t *idx_out, uint8_t *dist_out, void *stream) {
  if (!tokens || !planes128 || npad < n || npad % 256 || !lens || !slot_idx || !counts || !idx_out || !dist_out || n <= 0 || nrows <= 0 || row0 < 0 ||
      row0 + nrows > n || ld < l || cap < 0)
    return pg_fail(PG_E_BADARG, "pg_lev_knn: bad argument");
  if (int rc = check_l(l)) return rc;
  if (band < 0 || band > PG_LEV_MAX_BAND) return pg_fail(PG_E_BADARG, "pg_lev_knn: band must be in 0..8");
  if (k < 1 || k > PG_MAX_K) return pg_fail(PG_E_BADARG, "pg_lev_knn: k must be in 1..63");
  if (n > PG_MAX_N_KNN) return pg_fail(PG_E_TOOMANY, "pg_lev_knn: n exceeds 2^24");
  if (counts_lo && (row0 != 0 || nrows != n)) return pg_fail(PG_E_BADARG, "pg_lev_knn: symmetric slots cover all rows");
  return pg_launched(pg_launch_lev_select(tokens, n, l, ld, (const uint4 *)planes128, npad, lens, row0, nrows, band, k, (u32)cap, slot_idx, slot_w,
                                       slot_aux, counts, counts_lo, idx_out, dist_out, (hipStream_t)stream), "pg_lev_select_kernel");
}

// ---------------------------------------------------------------------------------------
// exact Levenshtein: dense matrix and the epsilon graph over symmetric candidate slots (pg_lev.hip)
// ---------------------------------------------------------------------------------------
int pg_levenshtein_dense(const void *x_planes128, int64_t n, int64_t x_npad, const int32_t *x_lens, const void *y_planes128,
                         int64_t m, int64_t y_npad, const int32_t *y_lens, int l, void *out, int out_elem_bytes, int64_t ldo,
                         void *stream) {
  if (!x_planes128 || !x_lens || !y_planes128 || !y_lens || !out || n <= 0 || m <= 0 || ldo < n)
    return pg_fail(PG_E_BADARG, "pg_levenshtein_dense: bad argument");
  if (l < 1 || l > PG_MAX_L) return pg_fail(PG_E_BADARG, "pg_levenshtein_dense: l must be in 1..128");
  if (out_elem_bytes != 2 && out_elem_bytes != 8) return pg_fail(PG_E_BADARG, "pg_levenshtein_dense: out_elem_bytes must be 2 or 8");
  if (x_npad < n || x_npad % 256 || y_npad < m) return pg_fail(PG_E_BADARG, "pg_levenshtein_dense: bad npad");
  if (((n + PG_WG_THREADS - 1) / PG_WG_THREADS) * ((m + PG_LEVD_ROWS - 1) / PG_LEVD_ROWS) > 0x7fffffffLL)
    return pg_fail(PG_E_TOOMANY, "pg_levenshtein_dense: too many blocks for one launch");
  return pg_launched(pg_launch_levenshtein_dense((const uint4 *)x_planes128, x_npad, n, x_lens, (const uint4 *)y_planes128, y_npad, m,
                                              y_lens, l, out, out_elem_bytes, ldo, (hipStream_t)stream),
                  "pg_levenshtein_dense_kernel");
}

int pg_lev_eps_pairs(const uint8_t *tokens, int64_t n, int l, int64_t ld, const void *planes128, int64_t npad,
                     const int32_t *lens, int band, int cap, const int32_t *slot_idx, uint8_t *slot_w, const int32_t *slot_aux,
                     const uint32_t *counts_up, const uint32_t *counts_lo, void *stream) {
  if (!tokens || !planes128 || !lens || !slot_idx || !slot_w || !slot_aux || !counts_up || !counts_lo || n <= 0 || ld < l ||
      cap < 0 || npad < n || npad % 256)
    return pg_fail(PG_E_BADARG, "pg_lev_eps_pairs: bad argument");
  if (l < 1 || l > PG_MAX_L) return pg_fail(PG_E_BADARG, "pg_lev_eps_pairs: l must be in 1..128");
  if (band < 0 || band > PG_LEV_MAX_BAND) return pg_fail(PG_E_BADARG, "pg_lev_eps_pairs: band must be in 0..8");
  return pg_launched(pg_launch_lev_pairs(tokens, n, l, ld, (const uint4 *)planes128, npad, lens, band, (u32)cap, slot_idx, slot_w,
                                      slot_aux, counts_up, counts_lo, (hipStream_t)stream), "pg_lev_select_kernel<1>");
}

static int lev_eps_args(int64_t n, int cap, int cmp, int thr, const char *who) {
  const int c = cmp & ~PG_CMP_KEEP_ZERO;
  if (n <= 0 || cap < 0 || (c != PG_CMP_LE && c != PG_CMP_LT && c != PG_CMP_EQ)) return pg_fail(PG_E_BADARG, who);
  if (thr < 0 || thr > PG_LEV_MAX_BAND) return pg_fail(PG_E_BADARG, "pg_lev_eps: the threshold must be in 0..8 (the band of the pairs)");
  return 0;
}

int pg_lev_eps_count(int64_t n, int cap, int cmp, int thr, const uint8_t *slot_w, const uint32_t *counts_up,
                     const uint32_t *counts_lo, uint32_t *counts_out, void *stream) {
  if (!slot_w || !counts_up || !counts_lo || !counts_out) return pg_fail(PG_E_BADARG, "pg_lev_eps_count: bad argument");
  if (int rc = lev_eps_args(n, cap, cmp, thr, "pg_lev_eps_count: bad argument")) return rc;
  return pg_launched(pg_launch_lev_eps(0, n, (u32)cap, cmp & ~PG_CMP_KEEP_ZERO, (u32)thr, (cmp & PG_CMP_KEEP_ZERO) ? 0u : 1u, nullptr,
                                    slot_w, counts_up, counts_lo, counts_out, nullptr, nullptr, nullptr, (hipStream_t)stream),
                  "pg_lev_eps_kernel<0>");
}

int pg_lev_eps_fill(int64_t n, int cap, int cmp, int thr, const int32_t *slot_idx, const uint8_t *slot_w,
                    const uint32_t *counts_up, const uint32_t *counts_lo, const int64_t *indptr, int32_t *indices,
                    uint8_t *weights, void *stream) {
  if (!slot_idx || !slot_w || !counts_up || !counts_lo || !indptr || !indices || !weights)
    return pg_fail(PG_E_BADARG, "pg_lev_eps_fill: bad argument");
  if (int rc = lev_eps_args(n, cap, cmp, thr, "pg_lev_eps_fill: bad argument")) return rc;
  return pg_launched(pg_launch_lev_eps(1, n, (u32)cap, cmp & ~PG_CMP_KEEP_ZERO, (u32)thr, (cmp & PG_CMP_KEEP_ZERO) ? 0u : 1u, slot_idx,
                                    slot_w, counts_up, counts_lo, nullptr, (const long long *)indptr, indices, weights,
                                    (hipStream_t)stream), "pg_lev_eps_kernel<1>");
}

int pg_csr_row_stats(const int64_t *indptr, const int32_t *indices, const uint8_t *weights_u8, const float *weights_f32,
                     int64_t nrows, int64_t row0, const double *f, double *deg, double *sum_f, double *sum_wf,
                     double *self_w, double *col_sum, void *stream) {
  if (!indptr || !indices || nrows <= 0 || row0 < 0) return pg_fail(PG_E_BADARG, "pg_csr_row_stats: bad argument");
  if ((sum_f || sum_wf) && !f) return pg_fail(PG_E_BADARG, "pg_csr_row_stats: node values required");
  pg_csr_row_stats_kernel<<<dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, (hipStream_t)stream>>>(
      (const long long *)indptr, indices, weights_u8, weights_f32, nrows, row0, f, deg, sum_f, sum_wf, self_w, col_sum);
  return pg_launched("pg_csr_row_stats_kernel");
}

int pg_compact_flags(const uint8_t *flags, int64_t n, int64_t *out_idx, int64_t *out_count, void *scratch,
                     void *stream) {
  if (!flags || !out_idx || !out_count || !scratch || n <= 0) return pg_fail(PG_E_BADARG, "pg_compact_flags: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const long long nb = (n + PG_SCAN_TILE - 1) / PG_SCAN_TILE;
  long long *part = (long long *)scratch;
  pg_scan_partials<unsigned char><<<dim3((unsigned)nb), dim3(256), 0, s>>>(flags, n, part);
  pg_scan_single<<<dim3(1), dim3(256), 0, s>>>(part, nb);
  pg_scan_apply<unsigned char, 1><<<dim3((unsigned)nb), dim3(256), 0, s>>>(flags, n, part, nb, (long long *)out_idx,
                                                                          (long long *)out_count);
  return pg_launched("pg_compact_flags");
}

// ---------------------------------------------------------------------------------------
// The path's one collective: all-gather of the row shards of the token matrix (e).
// RCCL is bound at run time: the copy the host process already carries (torch ships one as
// "librccl.so") or the ROCm installation's.  One communicator = one rank = one GPU (the current HIP
// device at pg_comm_init); the 128-byte id travels between the ranks by whatever channel the host has.
// ---------------------------------------------------------------------------------------
struct RcclApi {
  ncclResult_t (*GetUniqueId)(ncclUniqueId *);
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
  ncclResult_t (*CommDestroy)(ncclComm_t);
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
  const char *(*GetErrorString)(ncclResult_t);
};
static RcclApi *rccl() {
  static RcclApi api;
  static int state = 0;   // 0 untried, 1 ok, -1 missing
  static std::once_flag once;
  std::call_once(once, [&]() {
    void *h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);           // the host's copy, if it has one loaded
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (h) {
      api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(h, "ncclGetUniqueId");
      api.CommInitRank = (decltype(api.CommInitRank))dlsym(h, "ncclCommInitRank");
      api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
      api.AllGather = (decltype(api.AllGather))dlsym(h, "ncclAllGather");
      api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
    }
    state = (h && api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllGather) ? 1 : -1;
  });
  return state == 1 ? &api : nullptr;
}
static int rcclfail(RcclApi *r, ncclResult_t e, const char *where) {
  snprintf(g_err, sizeof(g_err), "%s: %s", where, r->GetErrorString ? r->GetErrorString(e) : "RCCL error");
  return PG_E_COMM;
}

int pg_comm_available(void) { return rccl() ? 1 : 0; }   // local, not a collective: can this process bind RCCL at all?

int pg_comm_unique_id(void *id128) {
  RcclApi *r = rccl();
  if (!r) return pg_fail(PG_E_COMM, "pg_comm_unique_id: librccl.so not found");
  if (!id128) return pg_fail(PG_E_BADARG, "pg_comm_unique_id: bad argument");
  ncclUniqueId id;
  ncclResult_t e = r->GetUniqueId(&id);
  if (e != ncclSuccess) return rcclfail(r, e, "ncclGetUniqueId");
  static_assert(sizeof(id) == PG_COMM_ID_BYTES, "ncclUniqueId size");
  memcpy(id128, &id, sizeof(id));
  return 0;
}

int pg_comm_init(void **comm, int nranks, int rank, const void *id128) {
  RcclApi *r = rccl();
  if (!r) return pg_fail(PG_E_COMM, "pg_comm_init: librccl.so not found");
  if (!comm || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return pg_fail(PG_E_BADARG, "pg_comm_init: bad argument");
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  ncclComm_t c = nullptr;
  ncclResult_t e = r->CommInitRank(&c, nranks, id, rank);
  if (e != ncclSuccess) return rcclfail(r, e, "ncclCommInitRank");
  *comm = (void *)c;
  return 0;
}

int pg_comm_destroy(void *comm) {
  RcclApi *r = rccl();
  if (!r || !comm) return pg_fail(PG_E_BADARG, "pg_comm_destroy: bad argument");
  ncclResult_t e = r->CommDestroy((ncclComm_t)comm);
  return e == ncclSuccess ? 0 : rcclfail(r, e, "ncclCommDestroy");
}

int pg_allgather_tokens(void *comm, const void *shard, int64_t rows_per_rank, int l, void *full, void *stream) {
  RcclApi *r = rccl();
  if (!r) return pg_fail(PG_E_COMM, "pg_allgather_tokens: librccl.so not found");
  if (!comm || !shard || !full || rows_per_rank <= 0 || l <= 0) return pg_fail(PG_E_BADARG, "pg_allgather_tokens: bad argument");
  ncclResult_t e = r->AllGather(shard, full, (size_t)rows_per_rank * (size_t)l, ncclUint8, (ncclComm_t)comm, (hipStream_t)stream);
  return e == ncclSuccess ? 0 : rcclfail(r, e, "ncclAllGather");
}

}  // extern "C"
