// step_lds_cfg.h -- what the planner (planner.cpp, plan_lds) and step_lds.hip (k_sweep_lds) agree on.
#pragma once

namespace sb {
namespace lds {

constexpr int kGuard = 16; // finite guard doubles before and after E in LDS

} // namespace lds
} // namespace sb
