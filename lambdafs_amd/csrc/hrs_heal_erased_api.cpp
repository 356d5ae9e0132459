// Heal with known erasures behind the C ABI (include/hrs.h): the erasure
// patterns of a batch (validated, de-duplicated, with the constants the
// kernels of hrs_heal_erased.hip multiply by), the device-resident call
// hrs_heal_erased_dev and one stripe on the CPU, hrs_heal_erased_host, the
// kernels' byte-exact reference. The per-column algorithm is
// locator::locate_errata (hrs_locator.hpp), the same code the kernels run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/hrs.h"
#include "gf256.hpp"
#include "hrs_codec.hpp"
#include "hrs_heal_erased.hpp"
#include "hrs_internal.hpp"
#include "hrs_locator.hpp"

namespace hrs::api {

namespace {

constexpr hrs::gf::Tables kHostTables = hrs::gf::make_tables();

// The erased set of one stripe: entries up to the first negative one (or
// `cap`), sorted ascending into `key`. HRS_EINVAL for a location outside
// [0, n) or a repeated one, HRS_ETOOMANY for more than p of them.
hrs_status erased_key(hrs_codec* c, const int* erased, int cap, size_t stripe, std::vector<int>& key) {
  key.clear();
  for (int t = 0; t < cap && erased[t] >= 0; ++t) {
    if (erased[t] >= c->n)
      return fail(c, HRS_EINVAL, "stripe %zu: erased location %d is outside [0, %d)", stripe, erased[t], c->n);
    key.push_back(erased[t]);
  }
  std::sort(key.begin(), key.end());
  for (size_t t = 1; t < key.size(); ++t)
    if (key[t] == key[t - 1]) return fail(c, HRS_EINVAL, "stripe %zu: erased location %d is listed twice", stripe, key[t]);
  if (static_cast<int>(key.size()) > c->p)
    return fail(c, HRS_ETOOMANY, "stripe %zu: %zu erased locations, the code repairs %d", stripe, key.size(), c->p);
  return HRS_OK;
}

// The device table entry of an erased set (hrs_heal_erased.hpp).
hrs::ErasePattern make_pattern(int p, const std::vector<int>& key) {
  const hrs::locator::Field f{kHostTables.exp, kHostTables.log};
  hrs::ErasePattern pt{};
  const int e = static_cast<int>(key.size()), pp = p - e;
  pt.e = e;
  for (int m = 0; m < e; ++m) {
    pt.loc[m] = static_cast<uint8_t>(key[m]);
    pt.mask[key[m] >> 5] |= 1u << (key[m] & 31);
  }
  while ((pt.mask[pt.spare >> 5] >> (pt.spare & 31)) & 1u) ++pt.spare;
  hrs::locator::erasure_locator(f, e, pt.loc, pt.gamma);
  uint8_t mat[hrs::locator::kMaxSyndromes][hrs::locator::kMaxSyndromes] = {};
  for (int o = 0; o < pp; ++o)
    for (int j = 0; j <= e; ++j) mat[o][o + e - j] = pt.gamma[j];
  if (e > 0) {
    std::vector<uint8_t> v(static_cast<size_t>(e) * e);  // v[i][m] = alpha^(loc[m] i)
    for (int i = 0; i < e; ++i)
      for (int m = 0; m < e; ++m) v[static_cast<size_t>(i) * e + m] = hrs::gf::alpha_pow(static_cast<long>(key[m]) * i);
    gf_invert(v, e);  // distinct locations: never singular
    for (int m = 0; m < e; ++m)
      for (int i = 0; i < e; ++i) mat[pp + m][i] = v[static_cast<size_t>(m) * e + i];
  }
  for (int i = 0; i < p; ++i)
    for (int o = 0; o < p; ++o) pt.cw[i] |= static_cast<uint64_t>(mat[o][i]) << (8 * o);
  return pt;
}

// One stripe on the CPU: the column loop of hrs_heal_erased_host.
template <int P>
void heal_erased_stripe(const hrs::locator::Field& f, int n, uint8_t* const* rows, size_t len,
                        const hrs::ErasePattern& pt, uint32_t* rep) {
  const int e = pt.e;
  for (size_t col = 0; col < len; ++col) {
    uint8_t s[P] = {};
    for (int l = n - 1; l >= 0; --l) {
      const bool gone = (pt.mask[l >> 5] >> (l & 31)) & 1u;
      hrs::locator::horner_step<P>(f, s, gone ? uint8_t{0} : rows[l][col]);
    }
    int nloc = 0;
    uint8_t loc[hrs::locator::kMaxErrors], u[hrs::locator::kMaxErrors], v[hrs::locator::kMaxErased];
    const int state = hrs::locator::locate_errata<P>(f, n, s, e, pt.loc, pt.gamma, &nloc, loc, u, v);
    for (int m = 0; m < e; ++m) rows[pt.loc[m]][col] = v[m];
    if (state == hrs::locator::kConsistent) continue;
    ++rep[HRS_SCRUB_BAD];
    if (rep[HRS_SCRUB_FIRST_BAD] == HRS_SCRUB_NONE) rep[HRS_SCRUB_FIRST_BAD] = static_cast<uint32_t>(col);
    if (state == hrs::locator::kUnresolved) {
      ++rep[HRS_SCRUB_UNRESOLVED];
      continue;
    }
    for (int j = 0; j < nloc; ++j) {
      ++rep[HRS_SCRUB_HEAD + loc[j]];
      if (u[j] == 0) continue;  // a blamed location whose value stands: nothing to store
      rows[loc[j]][col] ^= u[j];
      ++rep[HRS_SCRUB_PATCHED];
    }
  }
}

hrs_status run_heal_erased(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                           const std::vector<hrs::ErasePattern>& pats, const std::vector<int32_t>& pat,
                           uint32_t* reports, size_t report_stride, hipStream_t s) {
  const size_t pat_bytes = pats.size() * sizeof(hrs::ErasePattern);
  const size_t need = pat_bytes + pat.size() * sizeof(int32_t);
  hrs_codec::BatchSlot* sl = nullptr;
  hrs_status st = batch_slot_acquire(c, need, &sl);
  if (st != HRS_OK) return st;
  std::memcpy(sl->host, pats.data(), pat_bytes);
  std::memcpy(sl->host + pat_bytes, pat.data(), pat.size() * sizeof(int32_t));
  hipError_t e = hipMemcpyAsync(sl->dev, sl->host, need, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return hip_fail(c, e, "hipMemcpyAsync patterns");
  auto launches = [&]() -> hrs_status {
    e = hrs::launch_scrub_init(reports, report_stride, c->n, nstripes, s);
    if (e != hipSuccess) return hip_fail(c, e, "scrub init launch");
    hrs::HealErasedArgs a{};
    bool vec_ok = stride % 16 == 0 && c->kernel_mode != 2;
    for (int l = 0; l < c->n; ++l) {
      a.s.rows[l] = rows[l];
      vec_ok &= aligned16(rows[l]);
    }
    a.s.stride = stride;
    a.s.len = len;
    a.s.reports = reports;
    a.s.report_stride = report_stride;
    a.s.n = c->n;
    a.s.p = c->p;
    a.pats = reinterpret_cast<const hrs::ErasePattern*>(sl->dev);
    a.pat = reinterpret_cast<const int32_t*>(sl->dev + pat_bytes);
    a.s.nwin = vec_ok ? len / hrs::kWindowBytes : 0;
    if (a.s.nwin > 0) {
      a.s.ntasks = a.s.nwin * nstripes;
      e = hrs::launch_heal_erased(a, s);
      if (e != hipSuccess) return hip_fail(c, e, "heal erased launch");
      c->last_kernel = hrs::last_kernel();
    }
    a.s.col0 = a.s.nwin * hrs::kWindowBytes;
    if (a.s.col0 < len) {
      a.s.ntasks = (len - a.s.col0) * nstripes;
      e = hrs::launch_heal_erased_bytewise(a, s);
      if (e != hipSuccess) return hip_fail(c, e, "heal erased bytewise launch");
      if (a.s.nwin == 0) c->last_kernel = hrs::last_kernel();
    }
    return HRS_OK;
  };
  st = launches();
  // the slot's table may be in use whether or not every launch went out
  if (hipEventRecord(sl->done, s) == hipSuccess) sl->pending = true;
  else (void)hipStreamSynchronize(s);
  return st;
}

}  // namespace

}  // namespace hrs::api

using namespace hrs::api;

extern "C" {

hrs_status hrs_heal_erased_dev(hrs_codec* c, uint8_t* const* rows, size_t stride, size_t len, size_t nstripes,
                               const int* erased, int max_erased, uint32_t* reports, size_t report_stride,
                               void* stream) {
  if (!c) return HRS_EINVAL;
  hrs_status st = scrub_code_ok(c, report_stride, true);
  if (st != HRS_OK) return st;
  if (!rows || !reports) return fail(c, HRS_EINVAL, "rows or reports is NULL");
  st = heal_rows_ok(c, rows);
  if (st != HRS_OK) return st;
  if (max_erased < 0 || (max_erased > 0 && !erased))
    return fail(c, HRS_EINVAL, "max_erased %d with %s erased list", max_erased, erased ? "an" : "no");
  if (nstripes > 0x7fffffffu) return fail(c, HRS_EINVAL, "too many stripes");
  if (len > 0xffffffffu) return fail(c, HRS_EINVAL, "rows of %zu bytes: column indices are 32-bit", len);
  std::vector<hrs::ErasePattern> pats;
  std::vector<int32_t> pat(max_erased > 0 ? nstripes : 0, 0);
  if (max_erased > 0) {
    std::map<std::vector<int>, int32_t> ids;
    std::vector<int> key;
    for (size_t s = 0; s < nstripes; ++s) {
      st = erased_key(c, erased + s * static_cast<size_t>(max_erased), max_erased, s, key);
      if (st != HRS_OK) return st;
      auto it = ids.find(key);
      if (it == ids.end()) {
        it = ids.emplace(key, static_cast<int32_t>(pats.size())).first;
        pats.push_back(make_pattern(c->p, key));
      }
      pat[s] = it->second;
    }
  }
  if (len == 0 || nstripes == 0) return HRS_OK;
  DeviceGuard g(c->device);
  if (!g.ok) return fail(c, HRS_EDEVICE, "cannot select HIP device %d", c->device);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (max_erased == 0)  // nothing can be erased: the heal itself
    return run_scrub(c, rows, stride, len, nstripes, reports, report_stride, s, true);
  return run_heal_erased(c, rows, stride, len, nstripes, pats, pat, reports, report_stride, s);
}

hrs_status hrs_heal_erased_host(const hrs_codec* cc, uint8_t* const* rows, size_t len, const int* erased,
                                int num_erased, uint32_t* report) {
  auto* c = const_cast<hrs_codec*>(cc);
  if (!c) return HRS_EINVAL;
  hrs_status st = scrub_code_ok(c, 0, false);
  if (st != HRS_OK) return st;
  if (!rows || !report) return fail(c, HRS_EINVAL, "rows or report is NULL");
  st = heal_rows_ok(c, rows);
  if (st != HRS_OK) return st;
  if (num_erased < 0 || (num_erased > 0 && !erased))
    return fail(c, HRS_EINVAL, "num_erased %d with %s erased list", num_erased, erased ? "an" : "no");
  if (len > 0xffffffffu) return fail(c, HRS_EINVAL, "rows of %zu bytes: column indices are 32-bit", len);
  std::vector<int> key;
  st = erased_key(c, erased, num_erased, 0, key);
  if (st != HRS_OK) return st;
  if (len == 0) return HRS_OK;
  const hrs::ErasePattern pt = make_pattern(c->p, key);
  for (int e = 0; e < HRS_SCRUB_HEAD + c->n; ++e) report[e] = e == HRS_SCRUB_FIRST_BAD ? HRS_SCRUB_NONE : 0u;
  const hrs::locator::Field f{kHostTables.exp, kHostTables.log};
  switch (c->p) {
    case 1: heal_erased_stripe<1>(f, c->n, rows, len, pt, report); break;
    case 2: heal_erased_stripe<2>(f, c->n, rows, len, pt, report); break;
    case 3: heal_erased_stripe<3>(f, c->n, rows, len, pt, report); break;
    case 4: heal_erased_stripe<4>(f, c->n, rows, len, pt, report); break;
    case 5: heal_erased_stripe<5>(f, c->n, rows, len, pt, report); break;
    case 6: heal_erased_stripe<6>(f, c->n, rows, len, pt, report); break;
    case 7: heal_erased_stripe<7>(f, c->n, rows, len, pt, report); break;
    default: heal_erased_stripe<8>(f, c->n, rows, len, pt, report); break;
  }
  return HRS_OK;
}

}  // extern "C"
