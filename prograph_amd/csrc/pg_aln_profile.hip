// PROFILE (PSSM) queries: local, semi-global and fit alignment scores of position-specific score matrices against token
// sequences.  A profile is an (L, A) table, P[j][a] the score of aligning its position j with symbol a; the recurrences are
// those of pg_aln_local.hip, pg_aln_semiglobal.hip and pg_aln_fit.hip with S[x_i][y_j] replaced by P[j][x_i], the profile the
// Y operand: in fit mode ALL of the profile is placed within any stretch of the X row.  BUILD DEFINED.  DESIGN.md section 4.28.
//
// The token kernels turn every Y row into a byte query profile in LDS, Q[slot][a][j] = S[a][y_j] + bias, and their cell
// loops read nothing else of Y.  A PSSM is that query profile given, not gathered: the operand holds the bytes P + bias
// a-major with j contiguous, [profile][32][lpad], lpad a multiple of 128, zeros past a profile's length and for symbols
// the profile does not have, and the profile frames of pg_aln_frame.h copy it dword by dword into the 144-byte-stride rows.
// Modes, cell loop, saturating cells, boundary columns and the shift of fit scores are pg_aln_score.h's, unchanged.
//
// What the host passes in: bias = -min(0, min P) and top = max(0, max P) over the call's profiles (no reduction here),
// lengths as an int32 array (clamped to 0..yl here, so that no length reads outside the operand), and yl, the longest
// length, which stands where the width of the Y operand stands in the modes' offsets Z.  The exactness arguments of the
// three mode files hold with max P for max S - none of them uses the table's symmetry - and so do the caller's guarantees:
//     local        min(xl, yl) * top + 255 <= 65 535
//     semi-global  2 * min(xl, yl) * top + 255 <= 65 535
//     fit          gap_open + yl * (gap + 2 top) + 255 <= 65 535       (the short kernel too)
// The kernels do not test them.
#include "pg_aln_score.h"

template <class M, typename OUT>
__global__ __launch_bounds__(ALN_THREADS) __attribute__((amdgpu_waves_per_eu(3))) void pg_aln_profile_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ prof, const int *__restrict__ plen,
    int lpad4, long long m, int yl, u32 gap, u32 open, int obias, u32 bias, u32 top, OUT *__restrict__ out, long long ldo,
    long long colTiles) {
  aln_short_profile_frame<M>(xt, n, xnpad, xl, AlnProfiles{prof, plen, lpad4}, m, yl, gap, open, obias, bias, top, out, ldo, colTiles);
}

template <class M, typename OUT>
__global__ __launch_bounds__(ALN_THREADS) void pg_aln_profile_long_dense_kernel(
    const u32 *__restrict__ xt, long long n, long long xnpad, int xl, const u32 *__restrict__ prof, const int *__restrict__ plen,
    int lpad4, long long m, int yl, u32 gap, u32 open, int obias, u32 bias, u32 top, OUT *__restrict__ out, long long ldo,
    int colTiles, int items, u32 *ws) {
  aln_long_profile_frame<M>(xt, n, xnpad, xl, AlnProfiles{prof, plen, lpad4}, m, yl, gap, open, obias, bias, top, out, ldo, colTiles,
                            items, ws);
}

struct AlnProfileCall {            // what a profile entry has beyond an AlnCall (whose y: the profiles, table: the lengths)
  int mode, lpad, bias, top;
};

// the checks of aln_check, then the profile operand's; 0, or the error
static int aln_profile_check(const char *name, bool lng, const AlnCall &c, const AlnProfileCall &p, long long *colTiles, long long *items,
                             long long *blocks) {
  char msg[128];
  if (p.mode < 0 || p.mode > 2) {
    snprintf(msg, sizeof(msg), "%s: mode must be 0 (local), 1 (semi-global) or 2 (fit)", name);
    return pg_fail(PG_E_BADARG, msg);
  }
  if (const int rc = aln_check(name, lng, c, colTiles, items, blocks)) return rc;
  if (p.lpad % ALN_STRIP || p.lpad < c.yl || p.lpad > ALNG_MAX_L || p.bias < 0 || p.bias > 128 || p.top < 0 || p.top > 127) {
    snprintf(msg, sizeof(msg), "%s: lpad must be a multiple of 128 that covers yl, bias in 0..128, top in 0..127", name);
    return pg_fail(PG_E_BADARG, msg);
  }
  return 0;
}

template <class M, typename OUT>
static void aln_profile_short(const AlnCall &c, const AlnProfileCall &p, long long colTiles, long long blocks) {
  pg_aln_profile_dense_kernel<M, OUT><<<dim3((unsigned)blocks), dim3(ALN_THREADS), 0, (hipStream_t)c.stream>>>(
      (const u32 *)c.x, c.n, c.x_npad, c.xl, (const u32 *)c.y, (const int *)c.table, p.lpad / 4, c.m, c.yl, (u32)c.gap, (u32)c.gap_open,
      c.bias, (u32)p.bias, (u32)p.top, (OUT *)c.out, c.ldo, colTiles);
}

template <class M, typename OUT>
static void aln_profile_long(const AlnCall &c, const AlnProfileCall &p, long long colTiles, long long items, long long blocks) {
  pg_aln_profile_long_dense_kernel<M, OUT><<<dim3((unsigned)blocks), dim3(ALN_THREADS), 0, (hipStream_t)c.stream>>>(
      (const u32 *)c.x, c.n, c.x_npad, c.xl, (const u32 *)c.y, (const int *)c.table, p.lpad / 4, c.m, c.yl, (u32)c.gap, (u32)c.gap_open,
      c.bias, (u32)p.bias, (u32)p.top, (OUT *)c.out, c.ldo, (int)colTiles, (int)items, (u32 *)c.ws);
}

extern "C" {

int pg_alignment_profile_dense(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *profiles,
                               const int32_t *lengths, int64_t m, int lpad, int yl, int bias, int top, int gap, int gap_open,
                               int out_bias, void *out, int64_t ldo, int out_elem_bytes, void *stream) {
  const char *name = "pg_alignment_profile_dense";
  const AlnCall c = {x_packed, n, x_npad, xl, profiles, m, m, yl, lengths, gap, gap_open, out_bias, out, ldo, out_elem_bytes, nullptr, 0, stream};
  const AlnProfileCall p = {mode, lpad, bias, top};
  long long colTiles, items, blocks;
  if (const int rc = aln_profile_check(name, false, c, p, &colTiles, &items, &blocks)) return rc;
  const bool f16 = out_elem_bytes == 2;
  if (mode == 0) f16 ? aln_profile_short<AlnLocal, _Float16>(c, p, colTiles, blocks) : aln_profile_short<AlnLocal, long long>(c, p, colTiles, blocks);
  else if (mode == 1) f16 ? aln_profile_short<AlnSemiglobal, _Float16>(c, p, colTiles, blocks) : aln_profile_short<AlnSemiglobal, long long>(c, p, colTiles, blocks);
  else f16 ? aln_profile_short<AlnFit, _Float16>(c, p, colTiles, blocks) : aln_profile_short<AlnFit, long long>(c, p, colTiles, blocks);
  return pg_launched(name);
}

int pg_alignment_profile_long_dense(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *profiles,
                                    const int32_t *lengths, int64_t m, int lpad, int yl, int bias, int top, int gap, int gap_open,
                                    int out_bias, void *out, int64_t ldo, int out_elem_bytes, void *workspace,
                                    int64_t workspace_bytes, void *stream) {
  const char *name = "pg_alignment_profile_long_dense";
  const AlnCall c = {x_packed, n,   x_npad,         xl,        profiles,        m,     m, yl, lengths, gap, gap_open, out_bias,
                     out,      ldo, out_elem_bytes, workspace, workspace_bytes, stream};
  const AlnProfileCall p = {mode, lpad, bias, top};
  long long colTiles, items, blocks;
  if (const int rc = aln_profile_check(name, true, c, p, &colTiles, &items, &blocks)) return rc;
  const bool i32 = out_elem_bytes == 4;
  if (mode == 0) i32 ? aln_profile_long<AlnLocal, int>(c, p, colTiles, items, blocks) : aln_profile_long<AlnLocal, long long>(c, p, colTiles, items, blocks);
  else if (mode == 1) i32 ? aln_profile_long<AlnSemiglobal, int>(c, p, colTiles, items, blocks) : aln_profile_long<AlnSemiglobal, long long>(c, p, colTiles, items, blocks);
  else i32 ? aln_profile_long<AlnFit, int>(c, p, colTiles, items, blocks) : aln_profile_long<AlnFit, long long>(c, p, colTiles, items, blocks);
  return pg_launched(name);
}

}  // extern "C"
