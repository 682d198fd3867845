// sb_layout.h -- the few layout constants the host-only planner (planner.cpp) shares with the device code (sb_device.h).
#pragma once

namespace sb {

constexpr int kNScalOut = 16;        // scalars exported by sb_get_scalars
constexpr int kChunk = 8;            // sweep steps per software-pipelined chunk
constexpr int kPad = 8;              // doubles (bytes for cls) of padding around each grid in HBM
constexpr int kLdsCap = 160 * 1024;  // bytes of LDS a CU has (gfx950)

} // namespace sb
