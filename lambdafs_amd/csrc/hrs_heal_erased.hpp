// Heal with known erasures (hrs_heal_erased_dev, include/hrs.h): the interface
// between the host unit (hrs_scrub_api.cpp) and the kernels
// (hrs_heal_erased.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hrs_internal.hpp"

namespace hrs {

// One erasure set, a device table entry. With pp = p - e, the kernels' linear
// step tv = M S over the p syndromes of the survivors is packed like
// RowArgs::cw: byte o of cw[i] = M[o][i], where
//   rows o < pp       T_o    = sum_j gamma[j] S_{o+e-j}   (modified syndromes)
//   rows o = pp + m   v_m    = sum_{i<e} Vinv[m][i] S_i   (the value at loc[m])
// and Vinv is the inverse of the e x e Vandermonde matrix alpha^(loc[m] i).
struct ErasePattern {
  int32_t e;         // erased locations, 0..p
  uint32_t mask[8];  // bit l: location l is erased
  uint64_t cw[8];
  uint8_t loc[8];    // ascending
  uint8_t gamma[12]; // Gamma_0..Gamma_e
  uint32_t spare;    // the lowest surviving location (n > e: there is one)
};

struct HealErasedArgs {
  ScrubArgs s;               // rows are written: erased cells filled, survivors patched
  const ErasePattern* pats;  // device table
  const int32_t* pat;        // device: pattern index of each stripe
};

hipError_t launch_heal_erased(const HealErasedArgs& a, hipStream_t s);
hipError_t launch_heal_erased_bytewise(const HealErasedArgs& a, hipStream_t s);

// The listed form (checked repair, hrs_repair.hpp): the same two kernels over
// the stripes a device list names. list[0] = how many, read at kernel entry
// and clamped to nstripes; list[1 + i] = the i-th listed stripe, whose pattern
// is h.pats[that stripe] (h.pat is not read). An entry >= nstripes is skipped,
// never indexed with. h.s.ntasks is the upper bound nstripes * nwin (bytewise:
// nstripes * (len - col0)) the grid is sized for; blocks past count * nwin
// leave before they load anything.
struct HealListedArgs {
  HealErasedArgs h;
  const uint32_t* list;
  uint32_t nstripes;
  uint32_t pad_;
};

hipError_t launch_heal_listed(const HealListedArgs& a, hipStream_t s);
hipError_t launch_heal_listed_bytewise(const HealListedArgs& a, hipStream_t s);

}  // namespace hrs
