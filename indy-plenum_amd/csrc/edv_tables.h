// edv_tables.h -- which [S]B table set a batch runs against (edv_set_table_policy,
// edv_table_state), plain C++ so the CPU test harness (libedv_hostcheck.so)
// checks the same decision the library makes.
#pragma once
#include <stdint.h>

namespace edv {

// A batch of at least this many requests (one wave per SIMD of a whole MI355X)
// asks for the large set under the `auto` policy.
constexpr uint64_t kLargeTablesMin = 65536;

// The values of EDV_TABLES_AUTO / _COMPACT / _LARGE (include/edv.h).
enum TablePolicy { kTablesAuto = 0, kTablesCompact = 1, kTablesLarge = 2 };
enum TableSet { kSetNone = -1, kSetCompact = 0, kSetLarge = 1 };

struct TableChoice {
  int use;      // the set the batch runs against (kSetCompact / kSetLarge)
  int build;    // the set to build first because the context does not hold it, or kSetNone
  bool failed;  // the failed flag to keep when no build is attempted
};

// The set a batch of n requests uses under `policy` in a context that holds
// the compact and / or the large set.  `failed`: a build of the large set has
// failed and is not retried (sticky until the policy is set again, or a trim
// or release); a caller whose build of the large set fails sets the flag and
// asks again, and is then sent to the compact set.
//   auto     the large set once held, for every batch (a batch of
//            kLargeTablesMin requests asks for it); else the compact one
//   compact  always the compact set, never the large one
//   large    the large set; the compact one only after a failed build
inline TableChoice choose_tables(int policy, uint64_t n, bool have_compact, bool have_large, bool failed) {
  failed = failed && !have_large;  // moot once the set is there
  bool large;
  if (policy == kTablesCompact) large = false;
  else if (policy == kTablesLarge) large = have_large || !failed;
  else large = have_large || (n >= kLargeTablesMin && !failed);
  if (large) return {kSetLarge, have_large ? kSetNone : kSetLarge, failed};
  return {kSetCompact, have_compact ? kSetNone : kSetCompact, failed};
}

}  // namespace edv
