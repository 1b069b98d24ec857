// CPU check of the window the merge of the symmetric kNN sweep keeps of a lane's delivered keys (prograph_amd/csrc/pg_plan.h:
// sym_window_pop, sym_window_empty, sym_window_refill - the text pg_knn_sym_merge_kernel runs in its rounds).  Sixteen lanes
// of a row are simulated: every lane has its own sorted list (a record's last k + 1 keys) and sixteen sorted delivered keys;
// k + 1 rounds of "the smallest head wins and advances", the refill taken by all lanes where any lane's window is empty, as
// the kernel's ballot does.  The reference moves a lane's whole list down one place at every win (the rounds as they were).
// Same winners in the same order and the same keys left in every lane, at window widths 1, 2 and 4.
// No device, no runtime, no link against the library.  Last line: "window_check ok: ..." or "window_check FAILED: n".
#include "../../prograph_amd/csrc/pg_plan.h"

#include <stdio.h>
#include <algorithm>
#include <vector>

static int g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++g_checks;                                           \
    if (!(cond)) {                                        \
      if (++g_fail <= 40) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                     \
  } while (0)

static const uint32_t NONE = 0xFFFFFFFFu;
struct Row {
  std::vector<uint32_t> own[16];        // ascending, at most k + 1 each
  std::vector<uint32_t> delivered[16];  // ascending, at most 16 each
};

// the rounds as they were: every list moves down whole
static std::vector<uint32_t> reference(const Row &row, int k1, std::vector<uint32_t> (&left)[16]) {
  std::vector<uint32_t> own[16], winners;
  for (int b = 0; b < 16; ++b) {
    own[b] = row.own[b];
    left[b] = row.delivered[b];
    left[b].resize(16, NONE);
  }
  for (int r = 0; r < k1; ++r) {
    uint32_t m = NONE;
    for (int b = 0; b < 16; ++b) {
      if (!own[b].empty()) m = std::min(m, own[b][0]);
      m = std::min(m, left[b][0]);
    }
    winners.push_back(m);
    if (m == NONE) continue;
    for (int b = 0; b < 16; ++b) {
      if (!own[b].empty() && own[b][0] == m) own[b].erase(own[b].begin());
      if (left[b][0] == m) { left[b].erase(left[b].begin()); left[b].push_back(NONE); }
    }
  }
  return winners;
}

template <int W> static std::vector<uint32_t> windowed(const Row &row, int k1, std::vector<uint32_t> (&left)[16], long long *refills) {
  uint32_t d[16][16];
  int used[16], pos[16];
  std::vector<uint32_t> winners;
  for (int b = 0; b < 16; ++b) {
    for (int j = 0; j < 16; ++j) d[b][j] = j < (int)row.delivered[b].size() ? row.delivered[b][j] : NONE;
    used[b] = 0; pos[b] = 0;
  }
  for (int r = 0; r < k1; ++r) {
    uint32_t m = NONE;
    for (int b = 0; b < 16; ++b) {
      const uint32_t head = pos[b] < (int)row.own[b].size() ? row.own[b][pos[b]] : NONE;
      m = std::min(m, std::min(head, d[b][0]));
    }
    winners.push_back(m);
    const bool any = m != NONE;
    bool empty = false;
    for (int b = 0; b < 16; ++b) {
      const uint32_t head = pos[b] < (int)row.own[b].size() ? row.own[b][pos[b]] : NONE;
      if (any && head == m) ++pos[b];
      sym_window_pop<W>(d[b], used[b], any && d[b][0] == m);
      CHECK(used[b] >= 0 && used[b] <= W, "W %d lane %d: used %d", W, b, used[b]);
      empty = empty || sym_window_empty<W>(used[b]);
    }
    if (empty) {                                             // (the kernel's ballot: every lane of the wave runs the refill)
      ++*refills;
      for (int b = 0; b < 16; ++b) {
        sym_window_refill<W>(d[b], used[b]);
        CHECK(used[b] < W, "W %d lane %d: used %d behind a refill", W, b, used[b]);
      }
    }
  }
  // what a lane still holds: the window's live part, then the keys behind the window; the places wins vacated read "no entry"
  for (int b = 0; b < 16; ++b) {
    left[b].clear();
    for (int j = 0; j < W - used[b]; ++j) left[b].push_back(d[b][j]);
    for (int j = W - used[b]; j < W; ++j) CHECK(d[b][j] == NONE, "W %d lane %d: vacated place %d holds %08x", W, b, j, d[b][j]);
    for (int j = W; j < 16; ++j) left[b].push_back(d[b][j]);
    left[b].resize(16, NONE);
  }
  return winners;
}

static long long g_refills[5] = {0, 0, 0, 0, 0};
static void run(const char *name, const Row &row, int k1) {
  std::vector<uint32_t> refLeft[16], left[16];
  const std::vector<uint32_t> ref = reference(row, k1, refLeft);
  auto same = [&](int w, const std::vector<uint32_t> &got) {
    CHECK(got == ref, "%s, k + 1 = %d, W = %d: the winners differ", name, k1, w);
    for (int b = 0; b < 16; ++b) CHECK(left[b] == refLeft[b], "%s, k + 1 = %d, W = %d: lane %d keeps other keys", name, k1, w, b);
  };
  same(1, windowed<1>(row, k1, left, &g_refills[1]));
  same(2, windowed<2>(row, k1, left, &g_refills[2]));
  same(4, windowed<4>(row, k1, left, &g_refills[4]));
  // the winners are the row's smallest keys in order, "no entry" where they run out
  std::vector<uint32_t> all;
  for (int b = 0; b < 16; ++b) {
    all.insert(all.end(), row.own[b].begin(), row.own[b].end());
    all.insert(all.end(), row.delivered[b].begin(), row.delivered[b].end());
  }
  std::sort(all.begin(), all.end());
  all.resize(k1, NONE);
  CHECK(ref == all, "%s, k + 1 = %d: the reference is not the sorted prefix", name, k1);
}

static uint32_t g_seed = 12345u;
static uint32_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }
// n distinct keys in ascending order
static std::vector<uint32_t> distinct(int n) {
  std::vector<uint32_t> v;
  uint32_t at = rnd() % 50u;
  for (int i = 0; i < n; ++i) { v.push_back(at); at += 1u + rnd() % 50u; }
  return v;
}
// keys dealt to the lanes' lists: key i goes to the delivered keys (which >= 0) or the own list (-1 - which) of lane `lane`
static void deal(Row *row, const std::vector<uint32_t> &keys, const std::vector<int> &lane, const std::vector<bool> &own) {
  for (size_t i = 0; i < keys.size(); ++i) (own[i] ? row->own[lane[i]] : row->delivered[lane[i]]).push_back(keys[i]);
}

int main() {
  const int k1s[3] = {2, 17, 20};
  for (int k1 : k1s) {
    // one lane holds the 16, 17 and 20 smallest keys: sixteen delivered, the next ones its own; the other lanes larger keys
    for (int top : {16, 17, 20}) {
      const std::vector<uint32_t> keys = distinct(40);
      Row row;
      for (int i = 0; i < 40; ++i) {
        if (i < 16) row.delivered[3].push_back(keys[i]);
        else if (i < top) row.own[3].push_back(keys[i]);
        else ((i & 1) ? row.delivered : row.own)[(i & 15) == 3 ? 4 : (i & 15)].push_back(keys[i]);
      }
      run(top == 16 ? "one lane holds the 16 smallest" : (top == 17 ? "one lane holds the 17 smallest" : "one lane holds the 20 smallest"), row, k1);
    }
    // two lanes alternate: even ranks lane 2, odd ranks lane 9, delivered keys all
    {
      const std::vector<uint32_t> keys = distinct(32);
      Row row;
      for (int i = 0; i < 32; ++i) row.delivered[(i & 1) ? 9 : 2].push_back(keys[i]);
      run("two lanes alternate", row, k1);
    }
    // per-lane counts 0, 1, W, W + 1, 2 W, 15 and 16 for every W, in two orders of the lanes, keys dealt at random
    for (int turn = 0; turn < 2; ++turn) {
      const int counts[16] = {0, 1, 1, 2, 2, 3, 4, 4, 5, 8, 15, 16, 0, 16, 3, 15};
      Row row;
      std::vector<int> lane;
      for (int b = 0; b < 16; ++b)
        for (int j = 0; j < counts[turn ? 15 - b : b]; ++j) lane.push_back(b);
      const std::vector<uint32_t> keys = distinct((int)lane.size());
      for (size_t i = lane.size(); i > 1; --i) std::swap(lane[i - 1], lane[rnd() % i]);
      deal(&row, keys, lane, std::vector<bool>(lane.size(), false));
      run(turn ? "counts 0 .. 16, descending lanes" : "counts 0 .. 16", row, k1);
    }
    // every winner an own key (the delivered keys are larger, and none at all), every winner a delivered key
    for (int form = 0; form < 3; ++form) {
      const std::vector<uint32_t> keys = distinct(64);
      Row row;
      for (int i = 0; i < 64; ++i) {
        const bool first = i < 32;
        if (form == 0) (first ? row.own[i & 15] : row.delivered[i & 15]).push_back(keys[i]);
        else if (form == 1) { if (first) row.own[i & 15].push_back(keys[i]); }
        else (first ? row.delivered[i & 15] : row.own[i & 15]).push_back(keys[i]);
      }
      run(form == 0 ? "own keys win" : (form == 1 ? "own keys alone" : "delivered keys win"), row, k1);
    }
    // fewer than k + 1 keys in all: "no entry" wins the last rounds and moves nothing
    for (int n : {0, 1, k1 - 1}) {
      const std::vector<uint32_t> keys = distinct(n);
      Row row;
      for (int i = 0; i < n; ++i) ((i % 3) ? row.delivered[(5 * i) & 15] : row.own[(5 * i) & 15]).push_back(keys[i]);
      run("fewer keys than k + 1", row, k1);
    }
    // at random: the delivered keys crowd into a few lanes
    for (int it = 0; it < 300; ++it) {
      const int n = (int)(rnd() % 120u), lanes = 1 + (int)(rnd() % 16u);
      const std::vector<uint32_t> keys = distinct(n);
      Row row;
      for (int i = 0; i < n; ++i) {
        const int b = (int)(rnd() % (uint32_t)lanes);
        if (rnd() % 4u && row.delivered[b].size() < 16) row.delivered[b].push_back(keys[i]);
        else if ((int)row.own[b].size() < k1) row.own[b].push_back(keys[i]);
      }
      run("random", row, k1);
    }
  }
  // the narrow windows took the cold path, and more often the narrower
  CHECK(g_refills[1] > g_refills[2] && g_refills[2] > g_refills[4] && g_refills[4] > 0, "refills %lld %lld %lld", g_refills[1], g_refills[2], g_refills[4]);
  if (g_fail) { printf("window_check FAILED: %d\n", g_fail); return 1; }
  printf("window_check ok: %d checks, refills at W = 1, 2, 4: %lld %lld %lld\n", g_checks, g_refills[1], g_refills[2], g_refills[4]);
  return 0;
}
