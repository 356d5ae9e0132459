// Ragged scrub and heal (hrs_scrub_ragged.hip): hrs_scrub_dev / hrs_heal_dev
// over cells of which only the leading bytes hold data (include/hrs.h, "ragged
// scrub and heal"). Kernel arguments and launchers.
#pragma once
#include "hrs_internal.hpp"

namespace hrs {

// The scrub launch `s` plus the per-call length table in hops order: stripe i
// of the launch owns lens[i * (n + 1) ..): the lengths of its n cells, then the
// largest of them, so a window at or beyond every cell costs one scalar read.
struct ScrubRaggedArgs {
  ScrubArgs s;
  const uint32_t* lens;  // device table, at the launch's first stripe
};

inline size_t scrub_ragged_words(int n) { return static_cast<size_t>(n) + 1; }

// scrub_ragged_kernel<P, Heal> over the whole 2 KiB windows (s.nwin per row).
hipError_t launch_scrub_ragged(const ScrubRaggedArgs& a, bool heal, hipStream_t s);
// scrub_ragged_bytewise_kernel<P, Heal> over columns [s.col0, s.len): any alignment.
hipError_t launch_scrub_ragged_bytewise(const ScrubRaggedArgs& a, bool heal, hipStream_t s);

}  // namespace hrs
