// spatial_plan.cpp -- k_spatial's index tables (spatial.h) and sb_spatial_shape.  Host only, no HIP.
#include "spatial.h"

#include <algorithm>
#include <string>

namespace sb {

int spatial_shape(int H, int W, int pool_h, int pool_w, int *map_h, int *map_w, const char *who) {
  if (H < 1 || W < 1) return fail(SB_ERR_INVALID, std::string(who) + ": the grid needs H, W >= 1");
  if (pool_h < 1 || pool_w < 1) return fail(SB_ERR_INVALID, std::string(who) + ": pool_h and pool_w must be >= 1");
  *map_h = (int)(((long long)H + pool_h - 1) / pool_h);
  *map_w = (int)(((long long)W + pool_w - 1) / pool_w);
  return SB_OK;
}

int build_spatial_tables(int H, int W, bool transposed, int Z, const int *zone_off, const int *zone_cells,
                         const std::vector<int> &state_index, int state_len, int n_ring, int pool_h, int pool_w,
                         SpatialTables &out) {
  const char *who = "sb_spatial_attach";
  out = SpatialTables{};
  if (pool_h < 0 || pool_w < 0) return fail(SB_ERR_INVALID, std::string(who) + ": negative pool size");
  if ((pool_h == 0) != (pool_w == 0))
    return fail(SB_ERR_INVALID, std::string(who) + ": pool_h and pool_w are both 0 (zone statistics only) or both >= 1");
  const int N = H * W;
  if ((int)state_index.size() != N) return fail(SB_ERR_INVALID, std::string(who) + ": the handle has no state index");
  const int Hc = transposed ? W : H, Wc = transposed ? H : W; // the caller's grid
  // caller cell g0 = y * Wc + x  <->  handle cell (row x, column y) when transposed
  auto to_handle = [&](int g0) { return transposed ? (g0 % Wc) * W + g0 / Wc : g0; };
  auto to_caller = [&](int g) { return transposed ? (g % W) * Wc + g / W : g; };
  int bad = 0;
  auto source = [&](int g0) {
    const int cs = state_index[(size_t)to_handle(g0)];
    const int s = cs >= 0 ? cs : state_len + (-cs - 1);
    if (cs >= 0 ? cs >= state_len : -cs - 1 >= n_ring) bad = 1;
    return s;
  };

  out.zone_off.assign(zone_off, zone_off + Z + 1);
  out.zone_src.resize((size_t)zone_off[Z]);
  std::vector<int> cells;
  for (int z = 0; z < Z; ++z) {
    cells.clear();
    for (int i = zone_off[z]; i < zone_off[z + 1]; ++i) {
      if (zone_cells[i] < 0 || zone_cells[i] >= N) return fail(SB_ERR_INVALID, std::string(who) + ": zone cell outside the grid");
      cells.push_back(to_caller(zone_cells[i]));
    }
    std::sort(cells.begin(), cells.end());
    for (size_t k = 0; k < cells.size(); ++k) out.zone_src[(size_t)zone_off[z] + k] = source(cells[k]);
  }

  if (pool_h > 0) {
    SB_CHECK(spatial_shape(Hc, Wc, pool_h, pool_w, &out.map_h, &out.map_w, who));
    out.pool_h = pool_h; out.pool_w = pool_w;
    const int nt = out.map_h * out.map_w;
    const long long area = (long long)std::min(pool_h, Hc) * std::min(pool_w, Wc); // (a pool beyond the grid: one tile of the grid)
    out.tile_wave = (long long)pool_h * pool_w > kSpatialLaneTile ? 1 : 0;
    out.tile_cnt.resize((size_t)nt);
    if (out.tile_wave) {
      out.tile_off.reserve((size_t)nt + 1);
      out.tile_src.reserve((size_t)N);
    } else {
      out.tile_len = (int)area;
      out.tile_src.assign((size_t)out.tile_len * nt, -1);
    }
    for (int i = 0; i < out.map_h; ++i)
      for (int j = 0; j < out.map_w; ++j) {
        const int t = i * out.map_w + j;
        const int y1 = (int)std::min<long long>((long long)(i + 1) * pool_h, Hc);
        const int x1 = (int)std::min<long long>((long long)(j + 1) * pool_w, Wc);
        if (out.tile_wave) out.tile_off.push_back((int)out.tile_src.size());
        int k = 0;
        for (int y = i * pool_h; y < y1; ++y)
          for (int x = j * pool_w; x < x1; ++x, ++k) {
            const int s = source(y * Wc + x);
            if (out.tile_wave) out.tile_src.push_back(s);
            else out.tile_src[(size_t)k * nt + t] = s;
          }
        out.tile_cnt[(size_t)t] = k;
      }
    if (out.tile_wave) out.tile_off.push_back((int)out.tile_src.size());
  }
  if (bad) return fail(SB_ERR_INVALID, std::string(who) + ": a state index outside the building's state");
  return SB_OK;
}

} // namespace sb

extern "C" int sb_spatial_shape(int32_t H, int32_t W, int32_t pool_h, int32_t pool_w, int32_t *map_h, int32_t *map_w) {
  if (!map_h || !map_w) return fail(SB_ERR_INVALID, "sb_spatial_shape: null argument");
  int mh = 0, mw = 0;
  SB_CHECK(sb::spatial_shape(H, W, pool_h, pool_w, &mh, &mw, "sb_spatial_shape"));
  *map_h = mh; *map_w = mw;
  return SB_OK;
}
