// Banded (capped) Levenshtein kNN — BASELINE.json configs[4]; SURVEY.md §8 row a9.
// NOT IN THE REFERENCE: build-defined, parity unpinned (checked in tests against the oracle's
// `levenshtein_banded` / `orc_lev_knn`).
//
// Definition.  d(a,b) = min(edit_distance(a,b), band+1) over the non-zero prefixes of two
// zero-right-padded token rows; neighbours are ordered by (d, column index), rank 0 is dropped,
// ranks 1..k are returned — the same canonical rule as the Hamming kNN.
//
// Three stages:
//  1. pg_lev_profile_kernel: per sequence a 36-byte "bag" profile (32 symbol counts + length).
//  2. the all-pairs engine (pg_nsq.h) with BagMetric: every edit changes the count SAD by <= 2
//     and the length by <= 1, so  max(SAD, 2*|dlen|) <= 2*band  is a NECESSARY condition for
//     d <= band.  10 VALU ops per pair; survivors (ascending column order, exact counts) land
//     in per-row candidate slots exactly like the epsilon graph.
//  3. pg_lev_select_kernel: one wave per row, one candidate per lane: exact banded edit distance
//     with the bit-parallel diagonal-band recurrence of Myers / Hyyrö (one 17-bit delta vector
//     pair per lane, ~24 VALU ops per text character instead of 4 per DP cell x 17 cells), sorted
//     insertion of (d << 24 | column) keys into the 64-lane register list, then the ranks that no
//     candidate within the band fills are taken by the smallest column indices at distance band+1.
//
// The same file holds the two exact (uncapped) users of these pieces: pg_levenshtein_dense_kernel, the (M, N)
// edit-distance matrix by Myers' full bit-vector recurrence on a 128-bit pattern, and the epsilon graph
// (pg_lev_eps_kernel) that turns the pair-once distances of PHASE 1 into a CSR.
#include "pg_nsq.h"

#define PG_LEV_MAXL 128
#define PG_LEV_W 17          // diagonals kept: band <= 8

int pg_occ_nsq_bag() {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, pg_nsq_kernel<BagMetric, 2, PG_MODE_EPS>, PG_WG_THREADS, 0) !=
      hipSuccess)
    n = 0;
  return n;
}

int pg_launch_nsq_bag_sym(const NsqParams &p, int grid, hipStream_t s) {
  pg_nsq_kernel<BagMetric, 2, PG_MODE_EPS_SYM><<<dim3(grid), dim3(PG_WG_THREADS), 0, s>>>(p);
  return (int)hipGetLastError();
}

int pg_launch_nsq_bag(const NsqParams &p, int grid, hipStream_t s) {
  pg_nsq_kernel<BagMetric, 2, PG_MODE_EPS><<<dim3(grid), dim3(PG_WG_THREADS), 0, s>>>(p);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// stage 1: profiles.  One thread per sequence; record dwords 0..7 = counts of symbols 0..31
// (symbol 0 = padding is not counted), dword 8 = length in bytes 0 and 1.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pg_lev_profile_kernel(const unsigned char *__restrict__ tok, long long n, int l,
                                                             long long ld, u32 *__restrict__ prof, long long npad,
                                                             int *__restrict__ lens, u32 *flags) {
  const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
  if (s >= npad) return;
  u32 w[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) w[i] = 0;
  if (s < n) {
    const unsigned char *row = tok + s * ld;
    int len = 0;
    u32 bad = 0;
    for (int j = 0; j < l; ++j) {
      const u32 t = row[j];
      if (t > 31u) bad = 1u;
      if (t != 0) {
        if (len != j) bad = 1u;          // zeros must be trailing padding only
        ++len;
        const u32 sym = t & 31u;
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] += (i == (int)(sym >> 2)) ? (1u << (8 * (sym & 3u))) : 0u;
      }
    }
    w[8] = (u32)len | ((u32)len << 8);
    lens[s] = len;
    if (bad) atomicOr(flags, bad);
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) prof[((long long)(i >> 2) * npad + s) * 4 + (i & 3)] = w[i];
}

// ---------------------------------------------------------------------------------------
// stage 3: exact banded DP per candidate + kNN selection, one wave per row
// ---------------------------------------------------------------------------------------
struct LevParams {
  const unsigned char *tok;     // row-major tokens (the wave's own row is read from here)
  long long n, ld;
  int l;
  const uint4 *planes;          // the same tokens bit-sliced with 5 planes at width 128: chunk p = plane p
  long long npad;
  const int *lens;
  long long row0, nrows;
  int band, k;
  u32 cap;
  const int *slotIdx;
  unsigned char *slotW;  // phases 1/2: the exact distance of every candidate entry (both halves of a pair)
  const int *slotAux;    // phase 1: back position of a front entry's mirror (pg_lev_candidates_sym)
  const u32 *counts;
  const u32 *countsLo;   // symmetric candidate slots (pg_lev_candidates_sym): entries found from the other side, or null
  int *knnIdx;
  unsigned char *knnDist;
};

// Banded edit distance, bit-parallel (Hyyrö 2003, diagonal band).  The row sequence a is the
// "text" (wave uniform), the lane's candidate b the "pattern".  For text position j the window
// bit r stands for pattern row i = j - B + r (r = 0..2B); VP/VN are the vertical +1/-1 deltas of
// the previous column already shifted to this window, and per column
//     Eq[r] = (b[j-B+r] == a[j])
//     D0 = (((Eq & VP) + VP) ^ VP) | Eq | VN          diagonal delta is zero
//     HP = VN | ~(D0 | VP);   HN = D0 & VP            horizontal deltas
//     X  = D0 >> 1;   VN = X & HP;   VP = HN | ~(X | HP) | top
// The cell (lb, la) lies on diagonal kf = lb - la = window bit B + kf, and along a diagonal the
// value grows by 1 - D0[bit]: distance = |kf| + la - sum_j D0_j[B + kf].  Initial vectors encode
// D[i][0] = |i| for the sentinel-extended strings: VP = bits >= B, VN = bits < B.
// Eq comes from b's five 128-bit planes: the window is a funnel shift (v_alignbit) of two
// adjacent plane dwords, and "plane bit equals a's bit" is folded with v_bitop3 against a mask
// (0 / ~0 per plane of a[j]) that the wave precomputes once per row in LDS.
// PHASE 0: distances + selection in one go (rectangular candidate slots, or symmetric ones without
// the mirror table).  With symmetric slots and the mirror table every candidate PAIR is evaluated
// once: PHASE 1 computes the distance of each front entry (column > row) and stores it with the
// entry and with its mirror entry in the other row's slot; PHASE 2 only selects from the stored
// distances.
template <int PHASE>
__global__ __launch_bounds__(PG_WG_THREADS) void pg_lev_select_kernel(const LevParams p) {
  __shared__ uint4 amask[PG_WG_WAVES][PG_LEV_MAXL][2];   // per text position: masks of planes 0..3 | plane 4
  __shared__ u32 ldsF[PG_WG_WAVES][64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long lr = (long long)blockIdx.x * PG_WG_WAVES + wv;
  if (lr >= p.nrows) return;
  const long long row = p.row0 + lr;
  const int la = __builtin_amdgcn_readfirstlane(p.lens[row]);
  const int B = p.band;
  const u32 capd = (u32)B + 1u;
  const u32 wbits = 2u * (u32)B + 1u;
  const u32 top = 1u << (wbits - 1u);

  for (int j = lane; PHASE != 2 && j < PG_LEV_MAXL; j += 64) {
    const u32 t = j < p.l ? (u32)p.tok[row * p.ld + j] : 0u;
    amask[wv][j][0] = make_uint4(0u - (t & 1u), 0u - ((t >> 1) & 1u), 0u - ((t >> 2) & 1u), 0u - ((t >> 3) & 1u));
    amask[wv][j][1] = make_uint4(0u - ((t >> 4) & 1u), 0u, 0u, 0u);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint4 *am = &amask[wv][0][0] + opaque_zero();

  u32 lst = 0xFFFFFFFFu, thr = 0xFFFFFFFFu;            // sorted keys across lanes / (k+1)-th key
  // symmetric slots: `up` candidates (column > row) at the front, `lo` (column < row) at the back in
  // arbitrary order, the row itself in neither: it enters here as key (0, row).  Keys are totally
  // ordered and every insertion compares whole keys, so the order of arrival does not matter.
  const u32 up = p.counts[lr];
  const u32 lo = p.countsLo ? p.countsLo[lr] : 0u;
  if (p.countsLo && lane == 0) lst = (u32)row;
  const u32 cnt = PHASE == 1 ? up : up + lo;           // phase 1 walks the front entries only
  const u32 ncand = cnt < p.cap ? cnt : p.cap;         // host guarantees cnt <= cap (re-runs otherwise)

  for (u32 c0 = 0; c0 < ncand; c0 += 64) {
    const bool have = c0 + lane < ncand;
    const u32 ci = c0 + lane;
    const u32 spos = ci < up ? ci : p.cap - 1u - (ci - up);
    const int col = have ? p.slotIdx[lr * (long long)p.cap + spos] : 0;
    u32 result = capd;
    const long long sidx = lr * (long long)p.cap + spos;
    if constexpr (PHASE == 2) {
      if (have) result = p.slotW[sidx];                 // stored by phase 1 (through this entry or its mirror)
    } else {
      const int lb = have ? p.lens[col] : 0;
      u32 P[5][6];                                        // plane p as dwords [zero, w0, w1, w2, w3, zero]
  #pragma unroll
      for (int q = 0; q < 5; ++q) {
        const uint4 v = p.planes[(long long)q * p.npad + col];
        P[q][0] = 0u; P[q][1] = v.x; P[q][2] = v.y; P[q][3] = v.z; P[q][4] = v.w; P[q][5] = 0u;
      }
      const int kf = lb - la;
      const bool done = !have || kf > B || kf < -B;
      const u32 rbit = (u32)(B + (done ? 0 : kf));
      u32 VP = ((1u << wbits) - 1u) & ~((1u << B) - 1u);
      u32 VN = (1u << B) - 1u;
      u32 zsum = 0;                                       // number of columns with D0[rbit] = 1
      bool alive = true;                                  // some lane can still end within the band
      // window start in the zero-extended 192-bit plane: bit offset j - B - 1 + 32 (>= 24)
  #pragma unroll
      for (int seg = 0; seg < 5; ++seg) {
        int j0 = 32 * seg - 31 + B, j1 = 32 * seg + B;
        if (j0 < 1) j0 = 1;
        if (j1 > la) j1 = la;
        for (int j = j0; j <= j1 && alive; ++j) {
          const u32 sh = (u32)(j - B - 1 + 32) & 31u;
          const uint4 m03 = am[(j - 1) * 2];
          const u32 m4 = am[(j - 1) * 2 + 1].x;
          const u32 mk[5] = {m03.x, m03.y, m03.z, m03.w, m4};
          u32 Eq = ~(__builtin_amdgcn_alignbit(P[0][seg + 1], P[0][seg], sh) ^ mk[0]);
  #pragma unroll
          for (int q = 1; q < 5; ++q) {
            const u32 wq = __builtin_amdgcn_alignbit(P[q][seg + 1], P[q][seg], sh);
            Eq = __builtin_amdgcn_bitop3_b32(Eq, wq, mk[q], 0x90);       // Eq & ~(wq ^ mk)
          }
          const u32 t = (Eq & VP) + VP;
          const u32 D0 = __builtin_amdgcn_bitop3_b32(t, VP, Eq, 0xBE) | VN;       // ((t ^ VP) | Eq) | VN
          const u32 HP = __builtin_amdgcn_bitop3_b32(VN, D0, VP, 0xF1);  // VN | ~(D0 | VP)
          const u32 HN = D0 & VP;
          const u32 X = __builtin_amdgcn_ubfe(D0, 1u, wbits - 1u);
          VN = X & HP;
          VP = __builtin_amdgcn_bitop3_b32(HN, X, HP, 0xF1) | top;       // HN | ~(X | HP) | top
          zsum += __builtin_amdgcn_ubfe(D0, rbit, 1u);
          if ((j & 7) == 0) {
            // the diagonal value never decreases: stop once no live lane can stay within the band
            const u32 cur = (u32)(kf < 0 ? -kf : kf) + (u32)j - zsum;
            alive = __builtin_amdgcn_ballot_w64(!done && cur <= (u32)B) != 0;
          }
        }
      }
      if (!done && alive) {
        const u32 v = (u32)(kf < 0 ? -kf : kf) + (u32)la - zsum;
        result = v < capd ? v : capd;
      }
    }
    if constexpr (PHASE == 1) {
      if (have) {
        p.slotW[sidx] = (unsigned char)result;
        const u32 pb = (u32)p.slotAux[sidx];
        if (pb < p.cap) p.slotW[(long long)col * p.cap + (p.cap - 1u - pb)] = (unsigned char)result;
      }
      continue;
    }

    // candidates arrive in ascending column order: same sorted insertion as the Hamming kNN
    u64 m = __builtin_amdgcn_ballot_w64(have && result <= (u32)B);
    if (m) {
      const u32 key = (result << 24) | (u32)col;
      do {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        const u32 x = __builtin_amdgcn_readlane(key, j);
        if (x < thr) {
          const u32 cur = lst;
          const u32 pv = wave_shr1(cur, 0u);
          lst = (cur <= x) ? cur : (pv > x ? pv : x);
          thr = __builtin_amdgcn_readlane(lst, p.k);
        }
      } while (m);
    }
  }

  if constexpr (PHASE == 1) return;
  // ranks not filled by in-band candidates go to the smallest column indices at distance band+1
  // (all in-band columns are already in the list when it is not full, so "not a list member"
  // is the whole test).  All quantities below are wave uniform.
  const u32 limit = capd << 24;
  const int nv = __popcll(__builtin_amdgcn_ballot_w64(lst < limit && lane <= p.k));
  int placed = 0;
  for (int round = 0; round < 3 && nv + placed <= p.k; ++round) {
    const u32 j = (u32)(round * 64 + lane);
    bool member = false;
    for (int e = 0; e < nv; ++e) member = member || ((__builtin_amdgcn_readlane(lst, e) & 0x00FFFFFFu) == j);
    const bool ok = !member && (long long)j < p.n;
    const u64 fm = __builtin_amdgcn_ballot_w64(ok);
    const u32 slot = (u32)(nv + placed) + mask_rank(fm);
    __builtin_amdgcn_wave_barrier();
    if (ok && slot <= 63u) ldsF[wv][slot] = limit | j;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int upto = nv + placed + (int)__popcll(fm);
    if (lane >= nv + placed && lane < upto && lane <= 63) lst = ldsF[wv][lane];
    placed = upto - nv;
    if (fm == 0 && (long long)(round * 64 + 64) >= p.n) break;     // ran out of columns
  }
  if (lane >= 1 && lane <= p.k) {
    const long long o = lr * (long long)p.k + (lane - 1);
    p.knnIdx[o] = (lst == 0xFFFFFFFFu) ? -1 : (int)(lst & 0x00FFFFFFu);
    p.knnDist[o] = (unsigned char)(lst >> 24);
  }
}

int pg_launch_lev_profile(const unsigned char *tok, long long n, int l, long long ld, u32 *prof, long long npad,
                          int *lens, u32 *flags, hipStream_t s) {
  pg_lev_profile_kernel<<<dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, s>>>(tok, n, l, ld, prof, npad, lens, flags);
  return (int)hipGetLastError();
}

int pg_launch_lev_select(const unsigned char *tok, long long n, int l, long long ld, const uint4 *planes,
                         long long npad, const int *lens, long long row0,
                         long long nrows, int band, int k, u32 cap, const int *slotIdx, unsigned char *slotW,
                         const int *slotAux, const u32 *counts, const u32 *countsLo,
                         int *knnIdx, unsigned char *knnDist, hipStream_t s) {
  LevParams p;
  p.tok = tok; p.n = n; p.ld = ld; p.l = l; p.planes = planes; p.npad = npad; p.lens = lens; p.row0 = row0; p.nrows = nrows;
  p.band = band; p.k = k; p.cap = cap; p.slotIdx = slotIdx; p.slotW = slotW; p.slotAux = slotAux; p.counts = counts;
  p.countsLo = countsLo; p.knnIdx = knnIdx; p.knnDist = knnDist;
  const dim3 grid((unsigned)((nrows + PG_WG_WAVES - 1) / PG_WG_WAVES)), block(PG_WG_THREADS);
  if (countsLo && slotAux && slotW) {                   // every candidate pair once, then selection only
    pg_lev_select_kernel<1><<<grid, block, 0, s>>>(p);
    pg_lev_select_kernel<2><<<grid, block, 0, s>>>(p);
  } else {
    pg_lev_select_kernel<0><<<grid, block, 0, s>>>(p);
  }
  return (int)hipGetLastError();
}

int pg_launch_lev_pairs(const unsigned char *tok, long long n, int l, long long ld, const uint4 *planes, long long npad,
                        const int *lens, int band, u32 cap, const int *slotIdx, unsigned char *slotW, const int *slotAux,
                        const u32 *counts, const u32 *countsLo, hipStream_t s) {
  LevParams p;
  p.tok = tok; p.n = n; p.ld = ld; p.l = l; p.planes = planes; p.npad = npad; p.lens = lens; p.row0 = 0; p.nrows = n;
  p.band = band; p.k = 0; p.cap = cap; p.slotIdx = slotIdx; p.slotW = slotW; p.slotAux = slotAux; p.counts = counts;
  p.countsLo = countsLo; p.knnIdx = nullptr; p.knnDist = nullptr;
  pg_lev_select_kernel<1><<<dim3((unsigned)((n + PG_WG_WAVES - 1) / PG_WG_WAVES)), dim3(PG_WG_THREADS), 0, s>>>(p);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// epsilon graph from symmetric candidate slots whose distances PHASE 1 has stored: one wave per row.
// An entry is kept when comp(d, thr) and d >= dmin (1; 0 with PG_CMP_KEEP_ZERO).  A stored value is
// min(d, band+1) and thr <= band, so every kept value is the exact distance.  FILL = 0 counts the kept
// entries; FILL = 1 writes them at indptr[row] + rank, rank = number of kept entries of the row with a
// smaller column (columns are distinct within a row: every pair is a candidate once), which orders the
// back half of the slot - filled through atomics in arbitrary order - and the front half alike.
// ---------------------------------------------------------------------------------------
struct LevEpsParams {
  long long n;
  u32 cap, thr, dmin;
  int cmp;
  const int *slotIdx;
  const unsigned char *slotW;
  const u32 *counts, *countsLo;
  u32 *kept;                 // FILL = 0
  const long long *indptr;   // FILL = 1
  int *indices;
  unsigned char *weights;
};

template <int FILL>
__global__ __launch_bounds__(PG_WG_THREADS) void pg_lev_eps_kernel(const LevEpsParams p) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long row = (long long)blockIdx.x * PG_WG_WAVES + wv;
  if (row >= p.n) return;
  const u32 up = p.counts[row];
  const u32 all = up + p.countsLo[row];
  const u32 tot = all < p.cap ? all : p.cap;              // host guarantees all <= cap (re-runs otherwise)
  const long long base = row * (long long)p.cap;
  // entry e of the row: front part in slots [0, up), back part downwards from slot cap-1; a column that is
  // not kept reads as 0x7FFFFFFF, above every real column
  auto entry = [&](u32 e, u32 &d) -> u32 {
    d = 0;
    if (e >= tot) return 0x7FFFFFFFu;
    const long long o = base + (e < up ? e : p.cap - 1u - (e - up));
    d = p.slotW[o];
    const bool c = p.cmp == 0 ? d <= p.thr : (p.cmp == 1 ? d < p.thr : d == p.thr);
    return (c && d >= p.dmin) ? (FILL ? (u32)p.slotIdx[o] : 0u) : 0x7FFFFFFFu;   // counting needs no column
  };
  if constexpr (FILL == 0) {
    u32 cnt = 0;
    for (u32 e0 = 0; e0 < tot; e0 += 64) {
      u32 d;
      cnt += (u32)__popcll(__builtin_amdgcn_ballot_w64(entry(e0 + lane, d) != 0x7FFFFFFFu));
    }
    if (lane == 0) p.kept[row] = cnt;
  } else {
    const long long dst = p.indptr[row];
    if (p.indptr[row + 1] == dst) return;
    for (u32 e0 = 0; e0 < tot; e0 += 64) {
      u32 d;
      const u32 col = entry(e0 + lane, d);
      if (__builtin_amdgcn_ballot_w64(col != 0x7FFFFFFFu) == 0) continue;
      u32 rank = 0;
      for (u32 f0 = 0; f0 < tot; f0 += 64) {
        u32 df;
        const u32 cf = entry(f0 + lane, df);
        const int nf = (int)(tot - f0 < 64u ? tot - f0 : 64u);
        for (int t = 0; t < nf; ++t) rank += (u32)__builtin_amdgcn_readlane(cf, t) < col ? 1u : 0u;
      }
      if (col != 0x7FFFFFFFu) {
        p.indices[dst + rank] = (int)col;
        p.weights[dst + rank] = (unsigned char)d;
      }
    }
  }
}

int pg_launch_lev_eps(int fill, long long n, u32 cap, int cmp, u32 thr, u32 dmin, const int *slotIdx,
                      const unsigned char *slotW, const u32 *counts, const u32 *countsLo, u32 *kept,
                      const long long *indptr, int *indices, unsigned char *weights, hipStream_t s) {
  LevEpsParams p;
  p.n = n; p.cap = cap; p.thr = thr; p.dmin = dmin; p.cmp = cmp; p.slotIdx = slotIdx; p.slotW = slotW; p.counts = counts;
  p.countsLo = countsLo; p.kept = kept; p.indptr = indptr; p.indices = indices; p.weights = weights;
  const dim3 grid((unsigned)((n + PG_WG_WAVES - 1) / PG_WG_WAVES)), block(PG_WG_THREADS);
  if (fill) pg_lev_eps_kernel<1><<<grid, block, 0, s>>>(p);
  else pg_lev_eps_kernel<0><<<grid, block, 0, s>>>(p);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// dense exact edit distance: out[row][col] = d(Y[row], X[col]), no band, no cap.
// Myers' bit-vector recurrence in Hyyro's form, the X sequence b as the 128-bit pattern of one lane (five
// planes, four dwords each, kept in registers over PG_LEVD_ROWS rows of Y), the Y row a as the wave-uniform
// text, its per-position plane masks in LDS as in the banded kernel.  Per text position and dword
//     Eq = (b[i] == a[j])                                      v_xnor + 4 x v_bitop3
//     D0 = (((Eq & VP) + VP) ^ VP) | Eq | VN                   the + carries through the four dwords
//     HP = VN | ~(D0 | VP);   HN = D0 & VP
//     HP' = (HP << 1) | 1;  HN' = HN << 1                      shifts carry too; the 1 is D[0][j] - D[0][j-1]
//     VP = HN' | ~(D0 | HP');   VN = HP' & D0
// from VP = ~0, VN = 0 (D[i][0] = i).  Bit i depends on lower bits only, so pattern bits at and above lb (the
// padding, token 0, which no text symbol equals) never reach the rows that count, and the distance is read
// off the last column:  D[lb][la] = la + popcount(VP & rows) - popcount(VN & rows),  rows = bits below lb.
// The loop has no lane-dependent branch: its trip count is the text length.
// ---------------------------------------------------------------------------------------
struct LevDenseParams {
  const uint4 *xPlanes;
  long long xNpad, n;
  const int *xLens;
  const uint4 *yPlanes;
  long long yNpad, m;
  const int *yLens;
  int l;
  void *out;
  long long ldo, colTiles;
};

template <typename OUT>
__global__ __launch_bounds__(PG_WG_THREADS) void pg_levenshtein_dense_kernel(const LevDenseParams p) {
  __shared__ uint4 amask[PG_WG_WAVES][PG_LEV_MAXL][2];   // per text position: masks of planes 0..3 | plane 4
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long ct = (long long)blockIdx.x % p.colTiles, rg = (long long)blockIdx.x / p.colTiles;
  const long long col = (ct * PG_WG_WAVES + wv) * 64 + lane;      // < colTiles * 256 <= xNpad
  const bool have = col < p.n;
  int lb = have ? p.xLens[col] : 0;
  lb = lb < 0 ? 0 : (lb > p.l ? p.l : lb);
  u32 P[5][4], rows[4];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const uint4 v = p.xPlanes[(long long)q * p.xNpad + col];
    P[q][0] = v.x; P[q][1] = v.y; P[q][2] = v.z; P[q][3] = v.w;
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int nb = lb - 32 * w;
    rows[w] = nb >= 32 ? 0xFFFFFFFFu : (nb <= 0 ? 0u : (1u << nb) - 1u);
  }
  const uint4 *am = &amask[wv][0][0] + opaque_zero();

  for (int r = 0; r < PG_LEVD_ROWS; ++r) {
    const long long row = rg * PG_LEVD_ROWS + r;
    if (row >= p.m) break;
    int la = __builtin_amdgcn_readfirstlane(p.yLens[row]);
    la = la < 0 ? 0 : (la > p.l ? p.l : la);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // the previous row's reads are done
    __builtin_amdgcn_wave_barrier();
    for (int j = lane; j < PG_LEV_MAXL; j += 64) {
      u32 mk[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        const u32 *yw = (const u32 *)(p.yPlanes + (long long)q * p.yNpad + row);
        mk[q] = 0u - ((yw[j >> 5] >> (j & 31)) & 1u);
      }
      amask[wv][j][0] = make_uint4(mk[0], mk[1], mk[2], mk[3]);
      amask[wv][j][1] = make_uint4(mk[4], 0u, 0u, 0u);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    u32 VP[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, VN[4] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < la; ++j) {
      const uint4 m03 = am[j * 2];
      const u32 m4 = am[j * 2 + 1].x;
      u32 D0[4], HP[4], HN[4], carry = 0u;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        u32 Eq = ~(P[0][w] ^ m03.x);
        Eq = __builtin_amdgcn_bitop3_b32(Eq, P[1][w], m03.y, 0x90);        // Eq & ~(plane ^ mask)
        Eq = __builtin_amdgcn_bitop3_b32(Eq, P[2][w], m03.z, 0x90);
        Eq = __builtin_amdgcn_bitop3_b32(Eq, P[3][w], m03.w, 0x90);
        Eq = __builtin_amdgcn_bitop3_b32(Eq, P[4][w], m4, 0x90);
        const u32 t = __builtin_addc(Eq & VP[w], VP[w], carry, &carry);
        D0[w] = __builtin_amdgcn_bitop3_b32(t, VP[w], Eq, 0xBE) | VN[w];   // ((t ^ VP) | Eq) | VN
        HP[w] = __builtin_amdgcn_bitop3_b32(VN[w], D0[w], VP[w], 0xF1);    // VN | ~(D0 | VP)
        HN[w] = D0[w] & VP[w];
      }
#pragma unroll
      for (int w = 3; w >= 0; --w) {
        const u32 hp = w ? __builtin_amdgcn_alignbit(HP[w], HP[w - 1], 31) : ((HP[0] << 1) | 1u);
        const u32 hn = w ? __builtin_amdgcn_alignbit(HN[w], HN[w - 1], 31) : (HN[0] << 1);
        VP[w] = __builtin_amdgcn_bitop3_b32(hn, D0[w], hp, 0xF1);          // HN' | ~(D0 | HP')
        VN[w] = hp & D0[w];
      }
    }
    int d = la;
#pragma unroll
    for (int w = 0; w < 4; ++w) d += __popc(VP[w] & rows[w]) - __popc(VN[w] & rows[w]);
    if (have) ((OUT *)p.out)[row * p.ldo + col] = (OUT)d;
  }
}

int pg_launch_levenshtein_dense(const uint4 *xPlanes, long long xNpad, long long n, const int *xLens, const uint4 *yPlanes,
                                long long yNpad, long long m, const int *yLens, int l, void *out, int outBytes,
                                long long ldo, hipStream_t s) {
  LevDenseParams p;
  p.xPlanes = xPlanes; p.xNpad = xNpad; p.n = n; p.xLens = xLens; p.yPlanes = yPlanes; p.yNpad = yNpad; p.m = m;
  p.yLens = yLens; p.l = l; p.out = out; p.ldo = ldo;
  p.colTiles = (n + PG_WG_THREADS - 1) / PG_WG_THREADS;
  const long long blocks = p.colTiles * ((m + PG_LEVD_ROWS - 1) / PG_LEVD_ROWS);      // checked by pg_levenshtein_dense
  if (outBytes == 2) pg_levenshtein_dense_kernel<_Float16><<<dim3((unsigned)blocks), dim3(PG_WG_THREADS), 0, s>>>(p);
  else pg_levenshtein_dense_kernel<long long><<<dim3((unsigned)blocks), dim3(PG_WG_THREADS), 0, s>>>(p);
  return (int)hipGetLastError();
}
