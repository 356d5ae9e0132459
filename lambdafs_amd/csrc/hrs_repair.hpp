// Checked repair (hrs_repair_checked_dev, include/hrs.h): the interface
// between the host unit (hrs_repair_api.cpp) and the kernels of hrs_repair.hip.
// The listed heal kernels are hrs_heal_erased.hpp's (HealListedArgs).
//
// The call's scratch on the device, all of it written and read on the call's
// stream only:
//   list   uint32 [1 + nstripes]   word 0 = how many stripes are listed (zeroed
//                                  on the stream before the plan kernel), word
//                                  1 + i = the i-th listed stripe, in no order
//   pats   ErasePattern [nstripes] entry s = the table entry of stripe s, built
//                                  by the plan kernel when it lists s:
//                                  128 bytes per stripe of the batch
//   raw    uint32 [nstripes * n * ceil(len / 32 KiB)]  raw window CRCs of the
//                                  listed stripes, by place in the list
// Every kernel that reads the list clamps its count to nstripes and skips an
// entry >= nstripes without indexing anything with it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hrs_heal_erased.hpp"
#include "hrs_internal.hpp"

namespace hrs {

// repair_plan_kernel: one thread per stripe applies steps 1-3 of the rule
// (hrs_repair_rule.hpp) to pass 1's report and CRCs, writes the verdict and
// the erased_out row, and for a listed stripe builds pats[s], empties its
// report for pass 2 and appends s to the list (one atomic per wave).
struct RepairPlanArgs {
  const uint32_t* stored;   // [nstripes * n]
  const uint32_t* crcs;     // [nstripes * n], pass 1's crc_out
  uint32_t* reports;
  uint64_t report_stride;
  uint32_t* verdicts;       // [nstripes]
  int32_t* erased_out;      // [nstripes * p] or NULL
  uint32_t* list;
  ErasePattern* pats;
  uint32_t nstripes;
  int n, p, flags;
};
hipError_t launch_repair_plan(const RepairPlanArgs& a, hipStream_t s);

// repair_crc_window_kernel: crc_window_kernel's 32 KiB window walk over the
// cells of the listed stripes only: raw[(i * n + l) * wpr + w] for the i-th
// listed stripe, wpr = ceil(len / 32 KiB). The grid is sized for nstripes;
// blocks with nothing to do leave before they load the table image.
struct RepairCrcArgs {
  const uint8_t* rows[kScrubMaxRows];
  uint64_t stride;
  uint64_t len;
  const uint32_t* list;
  uint32_t nstripes;
  int n;
  int order;  // window -> wave order (task_order), set at launch
  int pad_;
  uint32_t* raw;
  const uint32_t* tables;  // kCrcLdsWordsA words (device)
};
hipError_t launch_repair_crc_windows(const RepairCrcArgs& a, bool aligned, int cus, hipStream_t s);

// repair_fold_verdict_kernel: one wave per listed stripe folds the raw window
// CRCs of its n cells (crc_fold_kernel's fold, fresh CRCs), compares each with
// the stored checksum and with pass 1's value it then overwrites in crc_out,
// and writes the stripe's verdict (step 6).
struct RepairFoldArgs {
  const uint32_t* raw;
  const uint32_t* list;
  const uint32_t* stored;
  uint32_t* crc_out;
  const uint32_t* reports;
  uint64_t report_stride;
  uint32_t* verdicts;
  uint64_t nwin;  // full 32 KiB windows per cell
  uint64_t tail;  // len - nwin * 32 KiB
  uint32_t nstripes;
  int n;
  int G;          // full windows per lane: ceil(nwin / 64)
  int pad_;
  const uint32_t* tables;  // kCrcLdsWordsB words (device), built for this len and 32 KiB windows
};
hipError_t launch_repair_fold_verdict(const RepairFoldArgs& a, int cus, hipStream_t s);

}  // namespace hrs
