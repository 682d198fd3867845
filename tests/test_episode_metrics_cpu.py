"""Episode totals per building without a device: csrc/episode_metrics.h (compiled for the host into a small program)
against its restatement ``host_inputs.EpisodeMetricsTwin``, equal bit for bit on random rows and at the edges; the twin
on the reference's recorded episodes; the header, the _ffi group and the names."""
import os
import re
import subprocess
import textwrap

import numpy as np
import pytest

from sbsim_amd import _ffi, host_inputs
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator, MixedBatchedEnvironment
from sbsim_amd.host_inputs import EpisodeMetricsTwin
from tests.golden_util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, S = _ffi.SB_EM_FIELDS, _ffi.SB_INFO_STRIDE
NAMES = _ffi.EPISODE_METRIC_NAMES

# stdin: "B Z dt" (dt as a hex double), then commands: "s" with, per building, the reward's bits (hex), the 24 info
# values' bits and the Z zone means' bits; "c" with B mask flags; "p" prints both tables' bits, running first.
PROGRAM = textwrap.dedent("""
    #include <cinttypes>
    #include <cstdio>
    #include <cstring>
    #include <vector>
    #include "episode_metrics.h"
    static float f32(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }
    static double f64(uint64_t u) { double x; std::memcpy(&x, &u, 8); return x; }
    struct Row { double v[SB_EM_FIELDS]; };
    int main() {
      int B, Z;
      double dt;
      if (std::scanf("%d %d %la", &B, &Z, &dt) != 3) return 1;
      std::vector<Row> run((size_t)B), done((size_t)B);
      for (int b = 0; b < B; ++b) { sb::metrics_init(run[b].v, 0.0); sb::metrics_init(done[b].v, -1.0); }
      char cmd[4];
      while (std::scanf("%3s", cmd) == 1) {
        if (cmd[0] == 's') {
          for (int b = 0; b < B; ++b) {
            uint32_t r, w;
            float info[SB_INFO_STRIDE];
            std::vector<double> zm((size_t)Z);
            if (std::scanf("%" SCNx32, &r) != 1) return 2;
            for (int k = 0; k < SB_INFO_STRIDE; ++k) { if (std::scanf("%" SCNx32, &w) != 1) return 2; info[k] = f32(w); }
            for (int z = 0; z < Z; ++z) { uint64_t v; if (std::scanf("%" SCNx64, &v) != 1) return 2; zm[z] = f64(v); }
            sb::metrics_step(run[b].v, f32(r), info, zm.data(), Z, dt);
          }
        } else if (cmd[0] == 'c') {
          for (int b = 0; b < B; ++b) {
            int m;
            if (std::scanf("%d", &m) != 1) return 2;
            if (m) sb::metrics_close(run[b].v, done[b].v);
          }
        } else {
          for (auto *t : {&run, &done})
            for (int b = 0; b < B; ++b)
              for (int k = 0; k < SB_EM_FIELDS; ++k) {
                uint64_t bits;
                std::memcpy(&bits, &(*t)[b].v[k], 8);
                std::printf("%016" PRIx64 "\\n", bits);
              }
        }
      }
      return 0;
    }
""")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
  d = tmp_path_factory.mktemp("episode_metrics")
  src, exe = os.path.join(d, "metrics.cpp"), os.path.join(d, "metrics")
  open(src, "w").write(PROGRAM)
  subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "sbsim_amd", "csrc"),
                  "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
  return exe


def _random_step(rng, B, Z, reject):
  """A step's outputs as k_post could write them: rates of either sign, small costs, counts, flags."""
  info = np.zeros((B, S), dtype=np.float32)
  info[:, :4] = rng.uniform(-5e4, 5e4, size=(B, 4))
  info[:, 4] = rng.randint(1, 101, size=B)
  info[:, 5] = rng.randint(0, 2, size=B)
  info[:, 6:] = rng.uniform(-3.0, 3.0, size=(B, S - 6))
  reward = rng.uniform(-2.0, 1.0, size=B).astype(np.float32)
  reward[reject] = -np.inf
  zm = rng.uniform(285.0, 305.0, size=(B, Z))
  return reward, info, zm


def _script(B, Z, dt, ops):
  """The program's input and the twin's tables for a list of ("s", reward, info, zm) / ("c", mask) / ("p",) ops."""
  twin = EpisodeMetricsTwin(B, dt)
  lines, want = [f"{B} {Z} {float(dt).hex()}"], []
  for op in ops:
    if op[0] == "s":
      _, reward, info, zm = op
      rows = []
      for b in range(B):
        words = [f"{int(reward[b:b + 1].view(np.uint32)[0]):x}"] + [f"{int(w):x}" for w in info[b].view(np.uint32)]
        words += [f"{int(w):x}" for w in np.ascontiguousarray(zm[b]).view(np.uint64)]
        rows.append(" ".join(words))
      lines.append("s " + " ".join(rows))
      twin.step(reward, info, zm)
    elif op[0] == "c":
      lines.append("c " + " ".join(str(int(m)) for m in op[1]))
      twin.close(op[1])
    else:
      lines.append("p")
      want.append(np.concatenate([twin.running.ravel(), twin.completed.ravel()]))
  return "\n".join(lines) + "\n", np.concatenate(want), twin


def _run(program, text):
  out = subprocess.run([program], input=text, check=True, capture_output=True, text=True).stdout.split()
  return np.array([int(x, 16) for x in out], dtype=np.uint64)


def _same_bits(got_bits, want):
  return np.array_equal(got_bits, np.ascontiguousarray(want, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("Z", [1, 4, 9])
def test_the_host_build_equals_the_twin_on_random_rows(program, Z):
  rng = np.random.RandomState(11 + Z)
  B = 6
  ops = [("p",)]                                                       # extremes before any step
  for t in range(9):
    ops.append(("s",) + _random_step(rng, B, Z, rng.rand(B) < 0.3))
    ops.append(("p",))
    if t in (3, 6):
      ops.append(("c", rng.rand(B) < 0.5))
      ops.append(("p",))
  text, want, twin = _script(B, Z, 300.0, ops)
  assert _same_bits(_run(program, text), want)
  assert (twin.completed[:, 1] > 0).any() and (twin.running[:, 0] > 0).any()   # something did close


def test_the_host_build_equals_the_twin_at_the_edges(program):
  rng = np.random.RandomState(5)
  B, Z = 4, 1
  # building 0 is rejected first, 1 in the middle, 2 last, 3 never
  rejects = [np.array([True, False, False, False]), np.array([False, True, False, False]), np.array([False, False, True, False])]
  ops = [("p",), ("c", np.ones(B, dtype=bool)), ("p",)]                 # extremes before a step; a close with steps == 0
  for r in rejects:
    ops += [("s",) + _random_step(rng, B, Z, r), ("p",)]
  ops += [("c", np.array([True, False, True, True])), ("p",), ("c", np.ones(B, dtype=bool)), ("p",)]   # ... and two in a row
  text, want, twin = _script(B, Z, 300.0, ops)
  got = _run(program, text)
  assert _same_bits(got, want)
  first = got[:2 * B * F].view(np.float64).reshape(2, B, F)
  assert (first[:, :, 18] == np.inf).all() and (first[:, :, 19] == -np.inf).all() and (first[0, :, 0] == 0).all()
  assert (first[1, :, 0] == -1).all() and (first[:, :, 1:18] == 0).all()
  after_empty_close = got[2 * B * F:4 * B * F]
  assert np.array_equal(after_empty_close, got[:2 * B * F])            # steps == 0: nothing closed, not a bit moved
  c = twin.completed
  assert np.isneginf(c[:3, 3]).all() and np.isfinite(c[3, 3]) and np.isfinite(c[:, 4]).all()
  assert c[:, 2].tolist() == [1, 1, 1, 0] and c[:, 1].tolist() == [3, 3, 3, 3]
  assert twin.running[:, 0].tolist() == [1, 1, 1, 1] and (twin.running[:, 1] == 0).all()


def test_the_twin_on_the_reference_episodes():
  g = load("h2_sb1_r9_episodes.npz")
  twin = EpisodeMetricsTwin(1, 300.0)
  for e, (ep, steps) in enumerate((("e1_", 14), ("e2_", 16))):
    rejected = g[ep + "rejected"].astype(bool)
    assert len(rejected) == steps
    for t in range(steps):
      info = np.zeros((1, S), dtype=np.float32)
      info[0, :4] = g[ep + "rates"][t]
      info[0, 4], info[0, 5] = g[ep + "n_sweeps"][t], 1.0
      info[0, 9], info[0, 10], info[0, 11] = g[ep + "rr_elec_cost"][t], g[ep + "rr_gas_cost"][t], g[ep + "rr_carbon"][t]
      reward = np.array([-np.inf if rejected[t] else g[ep + "reward"][t]], dtype=np.float32)   # environment.py:1301-1302
      twin.step(reward, info, g[ep + "zone_temp_post"][t][None, :])
    assert twin.close().all()
    row = dict(zip(NAMES, twin.completed[0]))
    assert row["episode"] == e and row["steps"] == steps and row["rejected_steps"] == rejected.sum() > 0
    assert np.isneginf(row["return"]) == bool(rejected.any()) and np.isneginf(row["return"])
    assert row["accepted_return"] == np.cumsum(g[ep + "reward"][~rejected].astype(np.float64))[-1]
    assert row["sweeps"] == g[ep + "n_sweeps"].sum() and row["unconverged_steps"] == 0
    assert row["zone_temp_min"] == g[ep + "zone_temp_post"].min() and row["zone_temp_max"] == g[ep + "zone_temp_post"].max()
    assert np.isclose(row["natural_gas_energy"], g[ep + "rates"][:, 2].astype(np.float64).sum() * 300.0 / 3.6e6, rtol=1e-12)
  assert twin.running[0, 0] == 2 and twin.running[0, 1] == 0


def test_the_twin_refuses_what_is_not_the_steps_float32():
  twin = EpisodeMetricsTwin(2, 300.0)
  with pytest.raises(ValueError, match="float32"):
    twin.step(np.zeros(2), np.zeros((2, S), dtype=np.float32), np.zeros((2, 3)))


def test_header_ffi_and_names_agree():
  header = open(os.path.join(ROOT, "include", "sbsim_amd.h")).read()
  assert re.search(r"#define SB_ABI_VERSION 8\b", header) and _ffi.SB_ABI_VERSION == 8
  assert int(re.search(r"#define SB_EM_FIELDS (\d+)", header).group(1)) == F == 20 == len(NAMES) == len(set(NAMES))
  enum = re.search(r"typedef enum sb_episode_metric \{(.*?)\} sb_episode_metric;", header, re.S).group(1)
  pairs = re.findall(r"SB_EM_([A-Z_]+) = (\d+)", enum)
  assert [(n.lower(), int(i)) for n, i in pairs] == [(n, i) for i, n in enumerate(NAMES)]
  for i, n in enumerate(NAMES):                                        # the documented table carries the same names
    assert re.search(rf"^ \*\s+{i} {n}\b", header, re.M), n
  for name in _ffi.EPISODE_METRICS_ENTRIES:
    assert re.search(rf"^int {name}\(", header, re.M), name
  assert set(_ffi.EPISODE_METRICS_ENTRIES) == {"sb_episode_metrics_attach", "sb_episode_metrics_detach", "sb_episode_metrics_get",
                                               "sb_episode_metrics_set"} <= set(_ffi.EXPORTS)
  assert "step_duration_sec" in header                                 # the reference's mislabelled series is named, not copied
  assert BatchedSimulator.EPISODE_METRIC_NAMES is NAMES is host_inputs.EPISODE_METRIC_NAMES
  assert BatchedEnvironment.EPISODE_METRIC_NAMES is NAMES is MixedBatchedEnvironment.EPISODE_METRIC_NAMES
  for cls in (BatchedSimulator, BatchedEnvironment, MixedBatchedEnvironment):
    assert callable(cls.episode_metrics) and callable(cls.completed_episodes)
  assert callable(BatchedSimulator.episode_metrics_attach) and callable(BatchedSimulator.episode_metrics_set)


def test_the_built_library_exports_the_group():
  lib = _ffi.load()
  for name in _ffi.EPISODE_METRICS_ENTRIES:
    assert hasattr(lib, name) and _ffi.episode_metrics_entry(name) is not None, name
  assert lib.sb_episode_metrics_get(None, None, None, None) == -1 and b"null argument" in lib.sb_last_error()
  assert lib.sb_episode_metrics_attach(None) == -1 and lib.sb_episode_metrics_detach(None) == -1
