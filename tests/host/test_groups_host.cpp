// The launch-group planner of the tempo and the beats call (bliss_amd/csrc/bl_groups.h) on the CPU: the properties of the
// rule on seeded random lists with small limits, so that every branch is taken many times, and one list worked out by
// hand from the rule (longest first, equal lengths in the caller's order; a new group starts at group_songs songs, or
// when a non-empty group would pass group_hops; hop_off == 0 marks a group's first record).
// Built and run by tests/test_groups_host.py: g++ -O2 -std=c++17, this header alone.
#include <stdio.h>

#include <random>
#include <vector>

#include "../../bliss_amd/csrc/bl_groups.h"

static int fails = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (++fails <= 20) {                    \
        printf("FAIL %s: ", #cond);           \
        printf(__VA_ARGS__);                  \
        printf("\n");                         \
      }                                       \
    }                                         \
  } while (0)

struct Rec { // what the planner needs of a record, and where the song stood in the caller's order
  long long hop_off;
  int hops;
  int idx;
};

struct Tally {
  long groups = 0, full = 0, by_hops = 0, over = 0;
};

// plans `hops` and checks every property; returns the records, `sizes` the song count of each group
static std::vector<Rec> plan(const std::vector<int> &hops, int group_songs, long long group_hops, int id,
                             std::vector<int> &sizes, Tally *tally) {
  const int n = (int)hops.size();
  std::vector<Rec> r(n);
  for (int i = 0; i < n; ++i) r[i] = Rec{-777, hops[i], i}; // the planner owns hop_off
  bl_groups_plan(r.data(), n, group_songs, group_hops);
  std::vector<int> seen(n, 0);
  for (int i = 0; i < n; ++i) {
    const bool inside = r[i].idx >= 0 && r[i].idx < n;
    CHECK(inside, "list %d: record %d has index %d", id, i, r[i].idx);
    if (!inside) return r;
    seen[r[i].idx] += 1;
    CHECK(r[i].hops == hops[r[i].idx], "list %d: record %d has %d hops, song %d had %d", id, i, r[i].hops, r[i].idx,
          hops[r[i].idx]);
    if (i) {
      CHECK(r[i].hops <= r[i - 1].hops, "list %d: %d hops behind %d", id, r[i].hops, r[i - 1].hops);
      CHECK(r[i].hops != r[i - 1].hops || r[i].idx > r[i - 1].idx, "list %d: equal hops, song %d behind song %d", id,
            r[i].idx, r[i - 1].idx);
    }
  }
  for (int i = 0; i < n; ++i) CHECK(seen[i] == 1, "list %d: song %d is there %d times", id, i, seen[i]);
  // the groups as the marks give them
  sizes.clear();
  CHECK(n == 0 || r[0].hop_off == 0, "list %d: the first record is no group start", id);
  for (int b = 0, e; b < n; b = e) {
    long long sum = r[b].hops;
    for (e = b + 1; e < n && r[e].hop_off != 0; ++e) {
      CHECK(r[e].hop_off == sum, "list %d: record %d at hop %lld, the group's earlier songs have %lld", id, e, r[e].hop_off,
            sum);
      sum += r[e].hops;
    }
    const int count = e - b;
    CHECK(count <= group_songs, "list %d: %d songs in a group, limit %d", id, count, group_songs);
    CHECK(sum <= group_hops || count == 1, "list %d: %d songs with %lld hops, limit %lld", id, count, sum, group_hops);
    CHECK(e == n || count == group_songs || sum + r[e].hops > group_hops,
          "list %d: song %d (%d hops) would have fitted behind %d songs with %lld hops", id, e, e < n ? r[e].hops : 0, count,
          sum);
    long long walked = -1;
    const int end = bl_group_end(r.data(), b, n, walked);
    CHECK(end == e && walked == sum, "list %d: group_end(%d) = %d with %lld hops, want %d with %lld", id, b, end, walked, e,
          sum);
    sizes.push_back(count);
    if (tally) {
      tally->groups += 1;
      if (e < n && count == group_songs) tally->full += 1;
      else if (e < n) tally->by_hops += 1;
      if (sum > group_hops) tally->over += 1;
    }
  }
  return r;
}

static void fixed(int group_songs, const std::vector<int> &want) {
  const std::vector<int> hops = {5, 9, 3, 9, 1, 4};
  std::vector<int> sizes;
  const std::vector<Rec> r = plan(hops, group_songs, 16, -group_songs, sizes, nullptr);
  printf("group_songs %d budget 16: %zu groups [", group_songs, sizes.size());
  for (size_t i = 0; i < sizes.size(); ++i) printf("%s%d", i ? "," : "", sizes[i]);
  printf("] order [");
  for (size_t i = 0; i < r.size(); ++i) printf("%s%d", i ? "," : "", r[i].idx);
  printf("]\n");
  CHECK(sizes == want, "group_songs %d", group_songs);
  const int order[6] = {1, 3, 0, 5, 2, 4}; // 9 (index 1), 9 (index 3), 5, 4, 3, 1
  for (int i = 0; i < 6; ++i) CHECK(r[i].idx == order[i], "group_songs %d: record %d is song %d", group_songs, i, r[i].idx);
}

int main() {
  std::mt19937_64 rng(20240911);
  const int lists = 4000;
  Tally t;
  std::vector<int> sizes;
  for (int id = 0; id < lists; ++id) {
    std::vector<int> hops(1 + (int)(rng() % 40));
    for (int &h : hops) h = 1 + (int)(rng() % 30);
    const int group_songs = 1 + (int)(rng() % 7);
    const long long group_hops = 1 + (long long)(rng() % 40);
    plan(hops, group_songs, group_hops, id, sizes, &t);
  }
  printf("%d lists, %ld groups: %ld ended at the song limit, %ld at the hop budget, %ld of one song above the budget\n",
         lists, t.groups, t.full, t.by_hops, t.over);
  CHECK(t.full > 1000 && t.by_hops > 1000 && t.over > 1000, "the random lists reach every branch of the rule");
  fixed(3, {1, 2, 3});
  fixed(2, {1, 2, 2, 1});
  // one song, and limits nothing reaches
  CHECK((plan({7}, 1, 1, -10, sizes, nullptr), sizes) == std::vector<int>({1}), "one song");
  CHECK((plan({5, 9, 3, 9, 1, 4}, 6, 31, -11, sizes, nullptr), sizes) == std::vector<int>({6}), "exact fit");
  CHECK((plan({5, 9, 3, 9, 1, 4}, 6, 30, -12, sizes, nullptr), sizes) == std::vector<int>({5, 1}), "one short of the fit");
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
