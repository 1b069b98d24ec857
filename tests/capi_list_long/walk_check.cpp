// Host-side check of the walk of the long list frame (prograph_amd/csrc/pg_aln_list_long.h) over its arithmetic
// (pg_aln_list_long_walk.h).  The four waves of a workgroup are walked one after the other through the frame's loops for
// one row - rounds outside, strip groups inside, the build between two barriers where a row has more than one group - for
// every list of 0..1100 entries and every strip count 0..16.  Checked: every entry of the list is visited exactly once, by
// a lane below 64; a wave runs all strips of a chunk, in order, before its next chunk (the workspace holds one boundary
// column per lane); a group's strips run only behind that group's build; all four waves reach the same number of
// barriers, the number aln_ll_barriers states; an empty list reaches none.  Test infrastructure; no GPU.
#include "pg_aln_list_long_walk.h"
#include <cstdio>
#include <vector>

static int bad = 0;
#define CHECK(c, ...)                      \
  do {                                     \
    if (!(c)) {                            \
      if (bad++ < 20) {                    \
        std::printf("FAILED %s: ", #c);    \
        std::printf(__VA_ARGS__);          \
        std::printf("\n");                 \
      }                                    \
    }                                      \
  } while (0)

int main() {
  long long rows = 0, visits = 0;
  for (int entries = 0; entries <= 1100; ++entries) {
    for (int ns = 0; ns <= 16; ++ns) {
      const int ly = ns ? ns * ALN_LL_STRIP - (entries + ns) % ALN_LL_STRIP : 0;      // any length with ns strips
      CHECK(aln_ll_strips(ly) == ns, "ly %d ns %d", ly, ns);
      std::vector<int> seen((size_t)entries, 0);                            // a block of exactly `entries`: a step outside is seen
      int barriers[ALN_LL_WAVES];
      const int chunks = aln_ll_chunks(entries);
      for (int wave = 0; wave < ALN_LL_WAVES; ++wave) {
        int &b = barriers[wave] = 0;
        if (chunks == 0) continue;                                          // the frame's `continue`: the whole workgroup
        b += 3;                                                             // tokens and length
        const bool regroup = aln_ll_groups(ns) > 1;
        int built = -1;                                                     // the group in the LDS slots
        if (!regroup) {
          built = 0;
          ++b;
        }
        for (int round = 0; round < aln_ll_rounds(chunks); ++round) {
          const int left = aln_ll_left(entries, round, wave);
          const bool active = left > 0;
          const long long eb = ((long long)round * ALN_LL_WAVES + wave) << 6;
          CHECK(left >= 0 && left <= 64, "left %d", left);
          int next_strip = 0;                                               // of this chunk
          for (int s0 = 0; s0 < ns; s0 += ALN_LL_SLOTS) {
            const int nb = ns - s0 < ALN_LL_SLOTS ? ns - s0 : ALN_LL_SLOTS;
            if (regroup) {
              b += 2;
              built = s0 / ALN_LL_SLOTS;
            }
            if (active)
              for (int s = s0; s < s0 + nb; ++s) {
                CHECK(s == next_strip && built == s / ALN_LL_SLOTS, "entries %d ns %d wave %d strip %d", entries, ns, wave, s);
                ++next_strip;
              }
          }
          CHECK(!active || next_strip == ns, "entries %d ns %d wave %d: %d strips", entries, ns, wave, next_strip);
          for (int l = 0; l < 64; ++l)
            if (l < left) {
              CHECK(eb + l < entries, "entry %lld of %d", eb + l, entries);
              if (eb + l < entries) ++seen[(size_t)(eb + l)];
              ++visits;
            }
        }
      }
      for (int wave = 0; wave < ALN_LL_WAVES; ++wave)
        CHECK(barriers[wave] == (chunks ? aln_ll_barriers(chunks, ns) : 0), "entries %d ns %d wave %d: %d barriers", entries, ns,
              wave, barriers[wave]);
      for (int e = 0; e < entries; ++e) CHECK(seen[(size_t)e] == 1, "entries %d ns %d: entry %d seen %d times", entries, ns, e, seen[(size_t)e]);
      ++rows;
    }
  }
  std::printf("%lld rows, %lld visits, %d failures\n", rows, visits, bad);
  if (!bad) std::printf("list long walk OK\n");
  return bad ? 1 : 0;
}
