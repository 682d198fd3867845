// planner_check.cpp -- the launch planner (sbsim_amd/csrc/planner.cpp) under the host sanitizers: it indexes its tables
// with unchecked operator[], and what it writes the sweep kernels trust.  A stand-alone program: planner.cpp and nothing
// else of the library, no GPU, not a test (tools/README.md has the command line).  It builds floor plans of its own --
// rectangular rooms on a grid inside an ambient ring, one class per (material, missing neighbours), zones = rooms,
// symmetric or asymmetric neighbour coefficients, with or without zone cells in the rows a tail scan would own -- from
// 4 x 4 to 300 x 420 cells, and plans each under every setting of the planner's switches.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "planner.h"

namespace {

struct Plan {
  int H = 0, W = 0, Z = 0;
  std::vector<uint8_t> cell_class;
  std::vector<double> class_coef;
  std::vector<int32_t> class_zone, zone_off, zone_cells;
  bool ok = true; // at most 255 classes
  sb_plan_desc desc() const {
    return sb_plan_desc{H, W, Z, (int32_t)class_zone.size(), cell_class.data(), class_coef.data(), class_zone.data(),
                        zone_off.data(), zone_cells.data()};
  }
};

// rows x cols cells inside a ring of one ambient cell; rooms of rh x rw cells between walls one cell thick.
// asym: the four neighbour coefficients of a class differ; tail_walls: the last two rows are wall (no zone cell there).
Plan make_plan(int rows, int cols, int rh, int rw, bool asym, bool tail_walls) {
  Plan p;
  p.H = rows + 2; p.W = cols + 2;
  const int rooms_across = (cols + rw) / (rw + 1);
  auto room_of = [&](int R, int C) { // -1: wall
    if (R % (rh + 1) == rh || C % (rw + 1) == rw || (tail_walls && R >= rows - 2)) return -1;
    return (R / (rh + 1)) * rooms_across + C / (rw + 1);
  };
  std::map<int, int> zone_id;                   // room -> zone, in raster order of the first cell
  std::map<std::pair<int, int>, int> class_id;  // (zone or -1, missing-neighbour mask) -> class
  std::vector<std::vector<int32_t>> cells;
  p.cell_class.assign((size_t)p.H * p.W, 0);
  p.class_coef = {0, 0, 0, 0, 0, 1.0, 0, 0};    // class 0: ambient (T' = T_ambient)
  p.class_zone = {-1};
  for (int R = 0; R < rows; ++R)
    for (int C = 0; C < cols; ++C) {
      const int room = room_of(R, C);
      int z = -1;
      if (room >= 0) {
        if (!zone_id.count(room)) { zone_id[room] = (int)cells.size(); cells.emplace_back(); }
        z = zone_id[room];
        cells[z].push_back((R + 1) * p.W + C + 1);
      }
      const int mask = (R == 0) | (R == rows - 1) << 1 | (C == 0) << 2 | (C == cols - 1) << 3;
      const auto key = std::make_pair(z, mask);
      if (!class_id.count(key)) {
        class_id[key] = (int)p.class_zone.size();
        const double b = z < 0 ? 0.05 : 0.2 + 0.001 * z; // a material per zone; walls conduct less
        for (int j = 0; j < 4; ++j) p.class_coef.push_back((mask >> j & 1) ? 0.0 : asym ? b * (1.0 - 0.1 * j) : b);
        const double rest[4] = {0.15, 0.0, z < 0 ? 0.0 : 0.01, 0.0}; // ap, gc, sc, spare
        p.class_coef.insert(p.class_coef.end(), rest, rest + 4);
        p.class_zone.push_back(z);
      }
      p.ok = p.ok && class_id[key] <= 255;
      p.cell_class[(size_t)(R + 1) * p.W + C + 1] = (uint8_t)class_id[key];
    }
  p.ok = p.ok && p.class_zone.size() <= 255;
  p.Z = (int)cells.size();
  p.zone_off.assign(1, 0);
  for (const auto &c : cells) {
    p.zone_cells.insert(p.zone_cells.end(), c.begin(), c.end());
    p.zone_off.push_back((int32_t)p.zone_cells.size());
  }
  if (p.zone_cells.empty()) p.zone_cells.push_back(0);
  return p;
}

struct Setting { const char *name[2], *value[2]; };
const Setting kSettings[] = {
    {{nullptr, nullptr}, {nullptr, nullptr}},
    {{"SBSIM_FORCE_LDS_PATH", nullptr}, {"1", nullptr}}, {{"SBSIM_FORCE_STREAM_PATH", nullptr}, {"1", nullptr}},
    {{"SBSIM_BAND_PATH", nullptr}, {"1", nullptr}}, {{"SBSIM_NO_TWO_ROW_PATH", nullptr}, {"1", nullptr}},
    {{"SBSIM_NO_TWO_ROW_PATH", "SBSIM_NO_BAND_PATH"}, {"1", "1"}}, {{"SBSIM_NO_ROLL_SMALL", nullptr}, {"1", nullptr}},
    {{"SBSIM_NO_ROLL_64", nullptr}, {"1", nullptr}}, {{"SBSIM_NO_TWO_64", nullptr}, {"1", nullptr}},
    {{"SBSIM_TWO_GENERAL", nullptr}, {"1", nullptr}}, {{"SBSIM_TWO_MAX_LEVEL", nullptr}, {"0", nullptr}},
    {{"SBSIM_TWO_MAX_LEVEL", nullptr}, {"1", nullptr}}, {{"SBSIM_DEBUG_LDS_PAD", nullptr}, {"30000", nullptr}},
};

} // namespace

int main() {
  // both sides of every limit of the kernels: 64 / 66 / 128 / 130 / 194 / 258 rows, 32 / 64 / 66 / 72 / 76 / 80 / 96 columns
  const int kRows[] = {2, 5, 17, 33, 47, 62, 63, 64, 65, 66, 67, 96, 127, 128, 129, 130, 131, 193, 194, 195, 257, 258, 259, 298};
  const int kCols[] = {2, 9, 31, 32, 33, 48, 63, 64, 65, 66, 67, 72, 73, 76, 77, 80, 81, 88, 95, 96, 97, 130, 250, 418};
  long long plans = 0, calls = 0, refused = 0, by_kernel[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t all = 0;
  int shape = 0;
  for (int rows : kRows)
    for (int cols : kCols) {
      ++shape;
      // rooms from one per plan to a few dozen (beyond the 31 zones k_sweep_roll's scratch takes), 1 .. 60 cells high
      const int rh = std::max(1, rows / (1 + shape % 7)), rw = std::max(1, cols / (1 + shape % 5));
      const Plan p = make_plan(rows, cols, rh, rw, shape % 3 == 1, shape % 3 != 2);
      if (!p.ok) continue;
      ++plans;
      const sb_plan_desc d = p.desc();
      if (sb::check_plan(&d) != SB_OK) { std::fprintf(stderr, "%d x %d: %s\n", p.H, p.W, sb::host::g_err.c_str()); return 1; }
      for (const Setting &s : kSettings)
        for (int per_building = 0; per_building < (s.name[0] ? 1 : 2); ++per_building) {
          for (int i = 0; i < 2; ++i)
            if (s.name[i]) setenv(s.name[i], s.value[i], 1);
          const sb::PlanKnobs k;
          sb::RegPlan r;
          sb::LdsPlan q;
          const int rc = sb::plan_sweep(&d, per_building != 0, "planner_check", k, r, q);
          for (int i = 0; i < 2; ++i)
            if (s.name[i]) unsetenv(s.name[i]);
          ++calls;
          if (rc != SB_OK) { ++refused; continue; }
          sb_launch_info info{};
          sb::fill_launch_info(&d, r, q, 3 * p.Z + 19, 256, 1024, &info);
          ++by_kernel[info.kernel];
          all = all * 1099511628211ull ^ sb::plan_digest(r, q);
        }
    }
  std::printf("planner_check: %lld plans, %lld calls, %lld refused; by kernel", plans, calls, refused);
  for (int kern = 0; kern < 7; ++kern) std::printf(" %lld", by_kernel[kern]);
  std::printf("; digest %016llx\n", (unsigned long long)all);
  return 0;
}
