// SPDX-License-Identifier: Apache-2.0
// The one reader of the library's CUDF_AMD_* settings (DESIGN.md appendix lists them). Read on every call, never cached: the
// test suite changes them between calls of one process.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace cudf::detail {

// The integer value of environment variable `name`; `dflt` if it is unset or empty.
inline int64_t env_i64(char const* name, int64_t dflt)
{
  char const* e = std::getenv(name);
  return (e != nullptr && *e != 0) ? std::strtoll(e, nullptr, 10) : dflt;
}

}  // namespace cudf::detail
