"""The seeded convection shuffle without a GPU: conv_seeded.h -- MT19937, CPython's seeding of an int and its three
consumers, the room pass -- compiled into a stand-alone program by the host compiler and held to Python's
``random.Random`` and to the reference's own permutations (tests/golden/convection_seeded.npz); the Python arguments,
the SimState round trip and the null-handle refusals of the four C entries."""
import ctypes as C
import os
import random
import subprocess
import textwrap

import numpy as np
import pytest

from sbsim_amd import _ffi, build
from tests.golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 11)
GOLDEN_CASES = (0, 1, 2)   # (1.0, 5, 7), (0.5, 3, 11), (1.0, -1, 5); cases 3 and 4 are windows of more than 64 offsets

PROGRAM = textwrap.dedent(r"""
    // Known answers of conv_seeded.h.  argv[1]: "draws" -- per seed of argv[2..] the seeded block, 2,000 interleaved
    // uniform / randbelow(1 + t % 37), a 777-element shuffle, the next raw word; "rooms" -- the room pass on the geometry
    // read from stdin: H W n_rooms, rooms as x0 y0 h w (in visiting order), n_calls, n_cases, cases as p distance seed.
    #include <cstdio>
    #include <cstdlib>
    #include <cstring>
    #include <vector>
    #include "conv_seeded.h"

    static int draws(int argc, char **argv) {
      for (int a = 2; a < argc; ++a) {
        sbconv::MtHost g(strtoull(argv[a], nullptr, 10));
        for (int k = 0; k < sbconv::kRngWords; ++k) printf("%u ", g.row[k]);
        printf("\n");
        for (int t = 0; t < 2000; ++t) {
          const double u = sbconv::uniform01(g);
          printf("%a %u ", u, sbconv::randbelow(g, 1u + (uint32_t)(t % 37)));
        }
        printf("\n");
        std::vector<int> x(777);
        for (int i = 0; i < 777; ++i) x[i] = i;
        sbconv::shuffle(g, x.data(), 777);
        for (int v : x) printf("%d ", v);
        printf("\n%u\n", g.next());
      }
      return 0;
    }

    static int rooms() {
      int H, W, R, calls, cases;
      if (scanf("%d %d %d", &H, &W, &R) != 3) return 2;
      std::vector<std::vector<int>> cells(R); // flat indices, raster order
      for (int r = 0; r < R; ++r) {
        int x0, y0, h, w;
        if (scanf("%d %d %d %d", &x0, &y0, &h, &w) != 4) return 2;
        for (int x = x0; x < x0 + h; ++x)
          for (int y = y0; y < y0 + w; ++y) cells[r].push_back(x * W + y);
      }
      if (scanf("%d %d", &calls, &cases) != 2) return 2;
      for (int c = 0; c < cases; ++c) {
        double p; int dist; unsigned long long seed;
        if (scanf("%lf %d %llu", &p, &dist, &seed) != 3) return 2;
        sbconv::MtHost g(seed);
        std::vector<double> temp((size_t)H * W);
        for (size_t i = 0; i < temp.size(); ++i) temp[i] = (double)i;
        for (int call = 0; call < calls; ++call) {
          for (int r = 0; r < R; ++r) {
            const int n = (int)cells[r].size();
            std::vector<int> rank((size_t)H * W, -1);
            for (int i = 0; i < n; ++i) rank[cells[r][i]] = i;
            std::vector<double> val(n);
            for (int i = 0; i < n; ++i) val[i] = temp[cells[r][i]];
            std::vector<uint32_t> rec(n);
            if (p == 1.0 && dist == -1) {
              for (int i = 0; i < n; ++i) rec[i] = (uint32_t)i;
              sbconv::shuffle(g, rec.data(), n);
              for (int i = 0; i < n; ++i) temp[cells[r][rec[i]]] = val[i];
              continue;
            }
            // every cell's in-room candidates in window raster order: row offset outside, column offset inside
            std::vector<std::vector<int>> cand(n);
            std::vector<int> cnt(n);
            for (int i = 0; i < n; ++i) {
              const int x = cells[r][i] / W, y = cells[r][i] % W;
              for (int dx = -dist; dx < dist; ++dx)
                for (int dy = -dist; dy < dist; ++dy) {
                  const int xx = x + dx, yy = y + dy;
                  if (xx < 0 || xx >= H || yy < 0 || yy >= W || dx * dx + dy * dy > dist) continue;
                  if (rank[xx * W + yy] >= 0) cand[i].push_back(rank[xx * W + yy]);
                }
              cnt[i] = (int)cand[i].size();
            }
            const int m = sbconv::room_draws(g, n, p, cnt.data(), rec.data());
            for (int k = 0; k < m; ++k) rec[k] = (rec[k] & 0xffff0000u) | (uint32_t)cand[rec[k] >> 16][rec[k] & 0xffffu];
            sbconv::shuffle(g, rec.data(), m);
            sbconv::room_swaps(rec.data(), m, val.data());
            for (int i = 0; i < n; ++i) temp[cells[r][i]] = val[i];
          }
          for (double v : temp) printf("%d ", (int)v);
          printf("\n");
        }
      }
      return 0;
    }

    int main(int argc, char **argv) {
      if (argc >= 2 && !strcmp(argv[1], "draws")) return draws(argc, argv);
      if (argc >= 2 && !strcmp(argv[1], "rooms")) return rooms();
      return 2;
    }
""")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
  d = tmp_path_factory.mktemp("conv_seeded")
  src, exe = os.path.join(d, "kat.cpp"), os.path.join(d, "kat")
  open(src, "w").write(PROGRAM)
  subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "sbsim_amd", "csrc"), src, "-o", exe],
                 check=True)
  return exe


def test_generator_seeding_and_consumers_equal_pythons_random(program):
  """MT19937 seeded the way CPython seeds an int (one or two 32-bit key words), then uniform(0, 1), _randbelow
  (randrange(n) is _randbelow(n)) and shuffle, draw for draw, and the raw word after them: the streams stay aligned."""
  out = subprocess.run([program, "draws", *(str(s) for s in SEEDS)], check=True, capture_output=True, text=True).stdout
  lines = out.strip().split("\n")
  assert len(lines) == 4 * len(SEEDS)
  for k, seed in enumerate(SEEDS):
    rng = random.Random(seed)
    words, draws, perm, raw = (lines[4 * k + i].split() for i in range(4))
    assert tuple(int(w) for w in words) == rng.getstate()[1] and int(words[624]) == 624, seed
    assert len(draws) == 4000
    for t in range(2000):
      u, r = rng.uniform(0, 1), rng.randrange(1 + t % 37)
      assert float.fromhex(draws[2 * t]).hex() == u.hex() and int(draws[2 * t + 1]) == r, (seed, t)
    x = list(range(777))
    rng.shuffle(x)
    assert [int(v) for v in perm] == x, seed
    assert int(raw[0]) == rng.getrandbits(32), seed


def test_room_pass_replays_the_reference_on_the_golden_geometry(program):
  """The golden's 14 x 26 grid with rooms of 9, 100 and 60 cells in first-appearance order, values = cell indices, three
  calls of cases 0-2: the grid after every call is the reference's own."""
  g = load("convection_seeded.npz")
  H, W = int(g["H"]), int(g["W"])
  rooms = sorted((tuple(int(v) for v in r) for r in g["rooms"]), key=lambda r: (r[0], r[1]))   # first cell, raster order
  assert sorted(h * w for _, _, h, w in rooms) == [9, 60, 100]
  calls = g["after"].shape[1]
  cases = [g["cases"][c] for c in GOLDEN_CASES]
  assert [(float(p), int(d), int(s)) for p, d, s in cases] == [(1.0, 5, 7), (0.5, 3, 11), (1.0, -1, 5)]
  text = f"{H} {W} {len(rooms)}\n" + "".join("%d %d %d %d\n" % r for r in rooms) + f"{calls} {len(cases)}\n"
  text += "".join(f"{float(p)!r} {int(d)} {int(s)}\n" for p, d, s in cases)
  out = subprocess.run([program, "rooms"], input=text, check=True, capture_output=True, text=True).stdout
  got = np.array([[int(v) for v in line.split()] for line in out.strip().split("\n")]).reshape(len(cases), calls, H, W)
  for i, c in enumerate(GOLDEN_CASES):
    for k in range(calls):
      assert np.array_equal(got[i, k], g["after"][c, k]), (c, k)
  assert not np.array_equal(got[0, 0], np.arange(H * W).reshape(H, W))


def test_seeded_simulator_argument_refusals():
  from sbsim_amd.host_inputs import SeededStochasticConvectionSimulator as S
  assert S(1.0, 5, 7).seeds_for(3).tolist() == [7, 8, 9] and S(1.0, 5, 7).seeds_for(3).dtype == np.uint64
  assert S(0.5, 3, [2 ** 64 - 1, 0, 2 ** 63 + 11]).seeds_for(3).tolist() == [2 ** 64 - 1, 0, 2 ** 63 + 11]
  assert S(1.0, -1, np.arange(4, dtype=np.int32)).seeds_for(4).tolist() == [0, 1, 2, 3]
  for bad in (1.5, np.array([1.0, 2.0]), "7", [True, False], None):
    with pytest.raises(ValueError, match="integer"):
      S(1.0, 5, bad)
  for bad in (np.zeros((2, 2), np.int64), np.zeros(0, np.int64), [[1, 2]]):
    with pytest.raises(ValueError, match="shape"):
      S(1.0, 5, bad)
  for bad in (-1, [3, -2], np.array([-5], np.int64)):
    with pytest.raises(ValueError, match="negative"):
      S(1.0, 5, bad)
  for bad in (2 ** 64, [1, 2 ** 64]):
    with pytest.raises(ValueError, match=r"below 2\^64"):
      S(1.0, 5, bad)
  with pytest.raises(ValueError, match="shape"):
    S(1.0, 5, [1, 2, 3]).seeds_for(4)
  with pytest.raises(ValueError, match=r"below 2\^64"):
    S(1.0, 5, 2 ** 64 - 2).seeds_for(3)


def test_sim_state_dict_round_trip_with_and_without_the_generators():
  import torch
  from sbsim_amd.environment import SimState
  n, Z, N = 2, 3, 12
  base = dict(grid=torch.rand(n, N, dtype=torch.float64), zone=torch.rand(n, 4, Z, dtype=torch.float64),
              mode=torch.zeros(n, Z, dtype=torch.int32), scal=torch.rand(n, _ffi.SB_STATE_NUM_SCALARS, dtype=torch.float64),
              nsw=torch.ones(n, dtype=torch.int32), occ=None, clock=(1, 2, 3, 1), fingerprint=((4, 3, Z), "x", ("seeded", 1.0, 5)))
  old = SimState(**base)
  assert old.conv_rng is None and "conv_rng" not in old.state_dict()     # what a checkpoint from before the option holds
  back = SimState.from_state_dict(old.state_dict(), "cpu")
  assert back.conv_rng is None and back.clock == old.clock and back.fingerprint == old.fingerprint
  rng = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, _ffi.SB_CONV_RNG_WORDS), dtype=torch.int32)
  new = SimState(**base, conv_rng=rng)
  d = new.state_dict()
  back = SimState.from_state_dict(d, "cpu")
  assert torch.equal(back.conv_rng, rng) and back.conv_rng.dtype == torch.int32 and torch.equal(back.grid, new.grid)
  assert back.fingerprint == new.fingerprint


def test_seeded_entries_refuse_a_null_handle():
  build.build()
  L = _ffi.load()
  assert set(_ffi.CONVECTION_SEEDED_ENTRIES) <= set(_ffi.EXPORTS)
  seeds = (C.c_uint64 * 2)(1, 2)
  attach = _ffi.convection_seeded_entry("sb_convection_attach_seeded")
  assert attach(None, 1.0, 5, seeds, 0) == -1 and b"null handle" in L.sb_last_error()
  buf = (C.c_uint32 * 625)()
  for name in ("sb_convection_rng_get", "sb_convection_rng_set"):
    assert _ffi.convection_seeded_entry(name)(None, C.cast(buf, C.c_void_p), None) == -1, name
    assert name.encode() in L.sb_last_error()
  assert _ffi.convection_seeded_entry("sb_convection_apply")(None, None) == -1 and b"null handle" in L.sb_last_error()
