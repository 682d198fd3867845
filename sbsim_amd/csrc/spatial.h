// spatial.h -- the index tables of k_spatial (spatial.hip), built on the host by spatial_plan.cpp.  Pure host arithmetic,
// no HIP, like planner.h: built and tested apart from the kernel.  The kernel trusts every index without checking.
#ifndef SBSIM_AMD_SPATIAL_H_
#define SBSIM_AMD_SPATIAL_H_

#include <cstdint>
#include <vector>

#include "sb_error.h"

namespace sb {

// Tiles of more cells than this are reduced by a wavefront in wave order, smaller ones by one lane in sequence
// (include/sbsim_amd.h, SUMMATION ORDER).  The rule reads pool_h * pool_w.
constexpr int kSpatialLaneTile = 64;

// A source index says where a control volume's value is: s < state_len -- element s of the building's state (doubles;
// float32 on a Jacobi handle); s >= state_len -- cell s - state_len of the building's exterior ring (register layouts),
// which reads scal[16] instead while scal[16] == scal[17] (k_copy_temps' rule).
struct SpatialTables {
  int pool_h = 0, pool_w = 0; // 0, 0: zone statistics only
  int map_h = 0, map_w = 0;   // tiles per column / row of tiles; n_tiles = map_h * map_w
  int tile_wave = 0;          // 1: pool_h * pool_w > kSpatialLaneTile
  int tile_len = 0;           // lane tiles: pool_h * pool_w, the rows of tile_src
  // lane tiles: [tile_len][n_tiles], entry k of tile t at k * n_tiles + t (lanes = tiles: coalesced), the tile's cells
  // row-major, then -1 up to tile_len (ragged tiles).  Wave tiles: the tiles' row-major lists back to back.
  std::vector<int> tile_src;
  std::vector<int> tile_off;  // wave tiles: [n_tiles + 1] into tile_src; lane tiles: empty
  std::vector<int> tile_cnt;  // [n_tiles] cells of the tile (the mean's divisor)
  std::vector<int> zone_off;  // [Z + 1] into zone_src
  std::vector<int> zone_src;  // per zone: its cells' source indices in ascending flat index of the CALLER's grid
};

int spatial_shape(int H, int W, int pool_h, int pool_w, int *map_h, int *map_w, const char *who);

// H, W: the HANDLE's grid (the transpose of the caller's when transposed != 0).  state_index: [H * W] per handle cell, >= 0
// an index into the state, < 0: -(ring cell + 1) (sb_handle::h_state_index).  zone_off / zone_cells: the handle's plan.
int build_spatial_tables(int H, int W, bool transposed, int Z, const int *zone_off, const int *zone_cells,
                         const std::vector<int> &state_index, int state_len, int n_ring, int pool_h, int pool_w,
                         SpatialTables &out);

} // namespace sb

#endif // SBSIM_AMD_SPATIAL_H_
