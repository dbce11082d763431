// The wave planner of the host-fed entry points (bliss_amd/csrc/bl_waves.h) on the CPU: the properties of the rule on
// seeded random length lists, and three splits of a fixed list worked out by hand from the rule (padded = (n + 7) & ~7;
// a song joins while total + padded <= budget; the first song of a wave always joins).
// Built and run by tests/test_waves_host.py: g++ -O2 -std=c++17, this header alone.
#include <stdio.h>
#include <stdint.h>

#include <random>
#include <vector>

#include "../../bliss_amd/csrc/bl_waves.h"

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

static size_t pad8(int32_t n) { return ((size_t)n + 7) & ~(size_t)7; }

// all waves of `n` under `budget`: the song count of each, every property checked on the way
static std::vector<int> split(const std::vector<int32_t> &n, size_t budget, int id) {
  std::vector<int> sizes;
  std::vector<size_t> off;
  const int count = (int)n.size();
  int covered = 0; // songs [0, covered) are in exactly one wave so far, in order
  for (int first = 0; first < count;) {
    size_t total = 12345;
    off.assign(3, 999); // the planner owns both outputs
    const int end = bl_wave_plan(n.data(), first, count, budget, off, total);
    CHECK(end > first && end <= count, "list %d: wave [%d, %d) of %d songs", id, first, end, count);
    if (end <= first || end > count) return sizes;
    CHECK(first == covered, "list %d: wave starts at %d, %d covered", id, first, covered);
    CHECK((int)off.size() == end - first, "list %d: %zu offsets for wave [%d, %d)", id, off.size(), first, end);
    if ((int)off.size() != end - first) return sizes;
    size_t want = 0; // songs back to back, each padded to 8: no overlap, no gap beyond the padding
    for (int i = first; i < end; ++i) {
      CHECK(off[i - first] % 8 == 0, "list %d: song %d at %zu", id, i, off[i - first]);
      CHECK(off[i - first] == want, "list %d: song %d at %zu, previous ends at %zu", id, i, off[i - first], want);
      want = off[i - first] + pad8(n[i]);
      CHECK(off[i - first] + (size_t)n[i] <= want, "list %d: song %d", id, i);
    }
    CHECK(total == want, "list %d: total %zu, songs end at %zu", id, total, want);
    CHECK(total <= budget || end - first == 1, "list %d: %d songs, %zu > budget %zu", id, end - first, total, budget);
    CHECK(end == count || total + pad8(n[end]) > budget, "list %d: song %d (%d) would have fitted %zu + . <= %zu", id,
          end, end < count ? n[end] : 0, total, budget);
    sizes.push_back(end - first);
    covered = end;
    first = end;
  }
  CHECK(covered == count, "list %d: %d of %d songs covered", id, covered, count);
  return sizes;
}

static void fixed(int rate, size_t budget, const std::vector<int> &want, int over_budget_wave) {
  static const int secs[13] = {1, 1, 2, 1, 3, 1, 1, 2, 1, 1, 3, 1, 1};
  std::vector<int32_t> n(13);
  for (int i = 0; i < 13; ++i) n[i] = rate * (1 + i % 2) * secs[i] + 8 * (i % 3);
  const std::vector<int> got = split(n, budget, -rate);
  printf("rate %d budget %zu: %zu waves [", rate, budget, got.size());
  for (size_t i = 0; i < got.size(); ++i) printf("%s%d", i ? "," : "", got[i]);
  printf("]\n");
  CHECK(got == want, "rate %d budget %zu", rate, budget);
  if (over_budget_wave >= 0 && got == want) {
    int first = 0;
    for (int w = 0; w < over_budget_wave; ++w) first += got[w];
    CHECK(got[over_budget_wave] == 1 && pad8(n[first]) > budget, "wave %d: song %d of %d samples", over_budget_wave, first,
          n[first]);
  }
}

int main() {
  std::mt19937_64 rng(20240611);
  const int lists = 4000;
  long waves = 0, singles_over = 0, multi = 0;
  for (int id = 0; id < lists; ++id) {
    const int count = 1 + (int)(rng() % 40);
    std::vector<int32_t> n(count);
    int32_t longest = 0;
    for (int &v : n) {
      // a third of the lists are short songs only, so that budgets of many songs occur too
      v = 1 + (int32_t)(rng() % (id % 3 == 0 ? 2000 : 200000));
      if (v > longest) longest = v;
    }
    const size_t budget = 1 + (size_t)(rng() % (4 * (uint64_t)longest));
    const std::vector<int> sizes = split(n, budget, id);
    waves += (long)sizes.size();
    int first = 0;
    for (int s : sizes) {
      if (s > 1) ++multi;
      else if (pad8(n[first]) > budget) ++singles_over;
      first += s;
    }
  }
  printf("%d lists, %ld waves: %ld of several songs, %ld of one song above the budget\n", lists, waves, multi,
         singles_over);
  CHECK(multi > 1000 && singles_over > 1000, "the random lists reach both branches of the rule");
  // budget 1 and a budget nothing exceeds
  CHECK(split({5, 9, 16, 1}, 1, -1) == std::vector<int>({1, 1, 1, 1}), "budget 1");
  CHECK(split({5, 9, 16, 1}, 8 + 16 + 16 + 8, -2) == std::vector<int>({4}), "exact fit");
  CHECK(split({5, 9, 16, 1}, 8 + 16 + 16 + 7, -3) == std::vector<int>({3, 1}), "one short of the fit");
  fixed(22050, 150000, {3, 2, 2, 2, 2, 2}, -1);
  fixed(44100, 150000, {2, 1, 1, 1, 2, 1, 2, 1, 2}, 5);
  fixed(44100, 75000, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, -1);
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("OK\n");
  return 0;
}
