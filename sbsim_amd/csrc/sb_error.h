// sb_error.h -- status codes with their sb_last_error() text, for every host translation unit (no HIP here: the planner
// reports through it too).
#pragma once

#include <string>

#include "sbsim_amd.h"

namespace sb {
namespace host {
inline thread_local std::string g_err; // sb_last_error()
} // namespace host
} // namespace sb

inline int fail(int code, const std::string &msg) {
  sb::host::g_err = msg;
  return code;
}

#define SB_CHECK(call)                                                                   \
  do {                                                                                   \
    const int rc_ = (call);                                                              \
    if (rc_ != SB_OK) return rc_;                                                        \
  } while (0)
