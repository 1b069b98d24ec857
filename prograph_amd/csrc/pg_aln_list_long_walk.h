// The arithmetic of the long list frame's walk (pg_aln_list_long.h) as plain functions of integers,
// in a header without HIP so that tests/capi_list_long can enumerate it on the host: a row's list of `entries` is cut into
// 64-entry chunks, walked in rounds of ALN_LL_WAVES chunks (wave w takes chunk ALN_LL_WAVES * round + w); the row's ly
// positions are cut into strips of ALN_LL_STRIP, ALN_LL_SLOTS strips to a group.
#pragma once

#if defined(__HIPCC__)
#define ALN_LL_FN static inline __host__ __device__
#else
#define ALN_LL_FN static inline
#endif

#define ALN_LL_WAVES 4             // = ALN_THREADS / 64
#define ALN_LL_STRIP 128           // = ALN_STRIP
#define ALN_LL_SLOTS 8             // = ALN_ROWS

// 64-entry chunks of a list of `entries`; 0 for an empty (or ill-formed, negative) one
ALN_LL_FN int aln_ll_chunks(long long entries) { return entries > 0 ? (int)((entries + 63) >> 6) : 0; }
// rounds of ALN_LL_WAVES chunks
ALN_LL_FN int aln_ll_rounds(int chunks) { return (chunks + ALN_LL_WAVES - 1) / ALN_LL_WAVES; }
// strips that hold a position of a row of ly positions, and groups of ALN_LL_SLOTS strips
ALN_LL_FN int aln_ll_strips(int ly) { return (ly + ALN_LL_STRIP - 1) / ALN_LL_STRIP; }
ALN_LL_FN int aln_ll_groups(int ns) { return (ns + ALN_LL_SLOTS - 1) / ALN_LL_SLOTS; }
// entries of wave w's chunk in round k: 0 when it has none
ALN_LL_FN int aln_ll_left(long long entries, int round, int wave) {
  const long long at = ((long long)round * ALN_LL_WAVES + wave) << 6;
  return at >= entries ? 0 : (int)(entries - at < 64 ? entries - at : 64);
}
// barriers every wave takes for one row with a list: 3 for the tokens and the length, then one after the build of a single
// group (an empty row's too), or two per (round, group) - whatever the wave's own chunks are
ALN_LL_FN int aln_ll_barriers(int chunks, int ns) {
  return 3 + (aln_ll_groups(ns) > 1 ? 2 * aln_ll_rounds(chunks) * aln_ll_groups(ns) : 1);
}
