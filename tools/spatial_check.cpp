// spatial_check.cpp -- k_spatial's index tables alone (sbsim_amd/csrc/spatial_plan.cpp, no HIP, no GPU) under the host
// sanitizers: a synthetic register-like layout (a permuted state index with padding, the border as ring cells), either
// orientation, nine pools on four grids.  Every index the kernel would follow must lie inside state + ring, every zone
// list must run in ascending caller index, every tile must list exactly its cells row-major, the tiles must cover the
// grid once.  Build machine only, not a test (tools/README.md has the command).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include "spatial.h"

using namespace sb;

static int check(int Hc, int Wc, bool tr, int ph, int pw, unsigned seed) {
  std::mt19937 rng(seed);
  const int H = tr ? Wc : Hc, W = tr ? Hc : Wc, N = H * W;
  // handle layout: border cells are ring cells, interior cells get a permuted state index with padding
  std::vector<int> sidx(N);
  int n_ring = 0;
  std::vector<int> interior;
  for (int g = 0; g < N; ++g) {
    const int y = g / W, x = g % W;
    if (y == 0 || x == 0 || y == H - 1 || x == W - 1) sidx[g] = -(n_ring++) - 1;
    else interior.push_back(g);
  }
  std::vector<int> perm(interior.size());
  std::iota(perm.begin(), perm.end(), 0);
  std::shuffle(perm.begin(), perm.end(), rng);
  const int state_len = (int)interior.size() + 7;
  for (size_t i = 0; i < interior.size(); ++i) sidx[interior[i]] = perm[i] + 3;
  // state values: value of handle cell g is g0 (its caller index) + 0.25
  auto to_caller = [&](int g) { return tr ? (g % W) * Wc + g / W : g; };
  std::vector<double> state(state_len, -1e9), ring(std::max(n_ring, 1), -1e9);
  for (int g = 0; g < N; ++g) {
    const double v = to_caller(g) + 0.25;
    if (sidx[g] >= 0) state[sidx[g]] = v; else ring[-sidx[g] - 1] = v;
  }
  // zones: two zones of interior cells (handle indices, ascending in the handle's raster)
  std::vector<int> zoff{0}, zc;
  for (int z = 0; z < 2; ++z) {
    for (int g : interior) if ((to_caller(g) % 3 == z)) zc.push_back(g);
    zoff.push_back((int)zc.size());
  }
  SpatialTables t;
  int rc = build_spatial_tables(H, W, tr, 2, zoff.data(), zc.data(), sidx, state_len, n_ring, ph, pw, t);
  if (rc != SB_OK) { printf("rc %d\n", rc); return 1; }
  auto val = [&](int s) {
    if (s < 0 || s >= state_len + n_ring) { printf("index out of range %d\n", s); exit(2); }
    return s < state_len ? state[s] : ring[s - state_len];
  };
  // zones: ascending caller index
  for (int z = 0; z < 2; ++z) {
    double prev = -1;
    for (int i = t.zone_off[z]; i < t.zone_off[z + 1]; ++i) {
      const double v = val(t.zone_src[i]);
      if (!(v > prev) || ((int)v % 3) != z) { printf("zone order\n"); return 1; }
      prev = v;
    }
    if (t.zone_off[z + 1] - t.zone_off[z] != zoff[z + 1] - zoff[z]) return 1;
  }
  if (ph == 0) return 0;
  const int nt = t.map_h * t.map_w;
  long long total = 0;
  for (int i = 0; i < t.map_h; ++i)
    for (int j = 0; j < t.map_w; ++j) {
      const int tt = i * t.map_w + j;
      std::vector<double> want;
      for (int y = i * ph; y < std::min<long long>((long long)(i + 1) * ph, Hc); ++y)
        for (int x = j * pw; x < std::min<long long>((long long)(j + 1) * pw, Wc); ++x) want.push_back(y * Wc + x + 0.25);
      std::vector<double> got;
      if (t.tile_wave) for (int k = t.tile_off[tt]; k < t.tile_off[tt + 1]; ++k) got.push_back(val(t.tile_src[k]));
      else for (int k = 0; k < t.tile_len; ++k) { const int s = t.tile_src[(size_t)k * nt + tt]; if (s >= 0) got.push_back(val(s)); }
      if (got != want || t.tile_cnt[tt] != (int)want.size()) { printf("tile %d %d mismatch\n", i, j); return 1; }
      total += (long long)want.size();
    }
  if (total != (long long)Hc * Wc) { printf("coverage\n"); return 1; }
  return 0;
}

int main() {
  int bad = 0, n = 0;
  const int pools[][2] = {{0, 0}, {1, 1}, {4, 4}, {5, 7}, {8, 8}, {9, 8}, {68, 98}, {1000, 3}, {2147483647, 2147483647}};
  const int shapes[][2] = {{68, 98}, {15, 23}, {7, 5}, {3, 3}};
  for (auto &s : shapes) for (auto &p : pools) for (int tr = 0; tr < 2; ++tr) { bad += check(s[0], s[1], tr, p[0], p[1], 7 + n); ++n; }
  SpatialTables t;
  std::vector<int> si(9, 0);
  int zo[1] = {0};
  bad += build_spatial_tables(3, 3, false, 0, zo, nullptr, si, 1, 0, -1, 2, t) != SB_ERR_INVALID;
  bad += build_spatial_tables(3, 3, false, 0, zo, nullptr, si, 1, 0, 0, 2, t) != SB_ERR_INVALID;
  si[4] = 5;
  bad += build_spatial_tables(3, 3, false, 0, zo, nullptr, si, 1, 0, 1, 1, t) != SB_ERR_INVALID; // index past the state
  printf("%d cases, %d bad\n", n, bad);
  return bad != 0;
}
