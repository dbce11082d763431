/*
 * bl_groups.h — how the tempo and the beats call (bl_feature_api.hip) cut the records of a call into launch groups:
 * longest first, as many songs as fit two limits but at least one.  Works on any record type with `hops` and `hop_off`
 * members.  Plain C++, no HIP: tests/host/test_groups_host.cpp compiles it alone.
 */
#ifndef BL_GROUPS_H_
#define BL_GROUPS_H_

#include <algorithm>

/* Sorts the n records longest first (equal lengths keep the caller's order) and cuts them into launch groups of at most
 * group_songs songs and group_hops hops; a song longer than that is a group of its own.  hop_off becomes the sum of
 * `hops` over the songs before it in its group, so hop_off == 0 marks the first song of a group: every song has
 * hops >= 1. */
template <class Rec>
void bl_groups_plan(Rec *recs, int n, int group_songs, long long group_hops) {
  std::stable_sort(recs, recs + n, [](const Rec &a, const Rec &b) { return a.hops > b.hops; });
  long long in_group = 0;
  for (int i = 0, count = 0; i < n; ++i, ++count) {
    if (count == group_songs || (count && in_group + recs[i].hops > group_hops)) in_group = count = 0;
    recs[i].hop_off = in_group;
    in_group += recs[i].hops;
  }
}

/* the end (one past the last record) of the group that starts at record b of n planned records; `hops`: its hops */
template <class Rec>
int bl_group_end(const Rec *recs, int b, int n, long long &hops) {
  int e = b + 1;
  for (hops = recs[b].hops; e < n && recs[e].hop_off; ++e) hops += recs[e].hops;
  return e;
}

#endif /* BL_GROUPS_H_ */
