/*
 * bl_waves.h — how the host-fed entry points (the host batch of bl_host_batch.hip, host_waves of bl_runtime.h under
 * every *_batch_host form) cut a list of songs into waves: songs in order, each at a multiple of 8 samples, as many as
 * fit a budget but at least one.  Plain C++, no HIP: tests/host/test_waves_host.cpp compiles it alone.
 */
#ifndef BL_WAVES_H_
#define BL_WAVES_H_

#include <stddef.h>
#include <stdint.h>

#include <vector>

/* The wave that starts at song `first` of n_songs: returns its end (one past its last song); offsets[i - first] is the
 * place of song i and `total` the wave's length with every song padded to 8, all in samples.  A song joins while the
 * padded total stays within `budget`; the first song always joins, so one song may exceed the budget. */
inline int bl_wave_plan(const int32_t *n_samples, int first, int n_songs, size_t budget, std::vector<size_t> &offsets,
                        size_t &total) {
  offsets.clear();
  total = 0;
  int end = first;
  for (; end < n_songs; ++end) {
    const size_t padded = ((size_t)n_samples[end] + 7) & ~(size_t)7;
    if (end > first && total + padded > budget) break;
    offsets.push_back(total);
    total += padded;
  }
  return end;
}

#endif /* BL_WAVES_H_ */
