"""Buildings scored against recorded zone temperatures without a device: csrc/telemetry.h (compiled for the host into a
small program, once more with -fsanitize=address,undefined) against its restatement ``host_inputs.TelemetryTwin``,
equal bit for bit on random rows and at the edges; what ``host_inputs.Telemetry`` refuses; the header, the _ffi group
and the names."""
import os
import re
import subprocess
import textwrap

import numpy as np
import pytest

from sbsim_amd import _ffi, host_inputs
from sbsim_amd.environment import BatchedEnvironment, BatchedSimulator, MixedBatchedEnvironment
from sbsim_amd.host_inputs import Telemetry, TelemetryTwin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, ZF = _ffi.SB_TL_FIELDS, _ffi.SB_TL_ZONE_FIELDS
NAMES = _ffi.TELEMETRY_SCORE_NAMES
COL = {n: i for i, n in enumerate(NAMES)}

# stdin: "B Z n_traces n_rows per_zone", the traces' bits (hex doubles, every row an allocation of its own: a read past a
# row is a heap overflow), B trace_of, B first_row, the Z weights' bits; then commands: "s" with the B * Z zone means'
# bits; "c" with B mask flags; "p" prints the scalar tables' bits (running, completed), with per_zone the per-zone
# tables' ([B][Z][4]: running, completed), then every building's action row as 16 hex digits.
PROGRAM = textwrap.dedent("""
    #include <cinttypes>
    #include <cstdio>
    #include <cstring>
    #include <vector>
    #include "telemetry.h"
    static double f64(uint64_t u) { double x; std::memcpy(&x, &u, 8); return x; }
    static void put(double x) { uint64_t u; std::memcpy(&u, &x, 8); std::printf("%016" PRIx64 "\\n", u); }
    struct Row { double v[SB_TL_FIELDS]; };
    int main() {
      int B, Z, NT, NR, PZ;
      if (std::scanf("%d %d %d %d %d", &B, &Z, &NT, &NR, &PZ) != 5) return 1;
      std::vector<std::vector<double>> rows((size_t)NT * NR, std::vector<double>((size_t)Z));
      for (auto &row : rows)
        for (int z = 0; z < Z; ++z) { uint64_t v; if (std::scanf("%" SCNx64, &v) != 1) return 2; row[z] = f64(v); }
      std::vector<int> trace_of((size_t)B), first_row((size_t)B);
      for (int b = 0; b < B; ++b) if (std::scanf("%d", &trace_of[b]) != 1) return 2;
      for (int b = 0; b < B; ++b) if (std::scanf("%d", &first_row[b]) != 1) return 2;
      std::vector<double> w((size_t)Z);
      for (int z = 0; z < Z; ++z) { uint64_t v; if (std::scanf("%" SCNx64, &v) != 1) return 2; w[z] = f64(v); }
      std::vector<Row> run((size_t)B), done((size_t)B);
      std::vector<std::vector<double>> zrun((size_t)B, std::vector<double>((size_t)Z * 4, 0.0)), zdone = zrun;
      for (int b = 0; b < B; ++b) { sb::telemetry_init(run[b].v, 0.0); sb::telemetry_init(done[b].v, -1.0); }
      char cmd[4];
      while (std::scanf("%3s", cmd) == 1) {
        if (cmd[0] == 's') {
          for (int b = 0; b < B; ++b) {
            std::vector<double> zm((size_t)Z);
            for (int z = 0; z < Z; ++z) { uint64_t v; if (std::scanf("%" SCNx64, &v) != 1) return 2; zm[z] = f64(v); }
            const double r = sb::telemetry_row(first_row[b], run[b].v[SB_TL_STEPS]);
            const double *tr = sb::telemetry_in_trace(r, NR) ? rows[(size_t)trace_of[b] * NR + (size_t)r].data() : nullptr;
            sb::telemetry_step(run[b].v, PZ ? zrun[b].data() : nullptr, 4, 1, zm.data(), tr, r, w.data(), Z);
          }
        } else if (cmd[0] == 'c') {
          for (int b = 0; b < B; ++b) {
            int m;
            if (std::scanf("%d", &m) != 1) return 2;
            if (m && sb::telemetry_close(run[b].v, done[b].v) && PZ) sb::telemetry_zone_close(zrun[b].data(), zdone[b].data(), 4, 1, Z);
          }
        } else {
          for (auto *t : {&run, &done})
            for (int b = 0; b < B; ++b)
              for (int k = 0; k < SB_TL_FIELDS; ++k) put((*t)[b].v[k]);
          if (PZ)
            for (auto *t : {&zrun, &zdone})
              for (int b = 0; b < B; ++b)
                for (double x : (*t)[b]) put(x);
          for (int b = 0; b < B; ++b)
            std::printf("%016" PRIx64 "\\n", (uint64_t)sb::telemetry_action_row(first_row[b], run[b].v[SB_TL_STEPS], NR));
        }
      }
      return 0;
    }
""")


def _compile(d, name, extra):
  src, exe = os.path.join(d, "telemetry.cpp"), os.path.join(d, name)
  open(src, "w").write(PROGRAM)
  subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", *extra,
                  "-I", os.path.join(ROOT, "sbsim_amd", "csrc"), "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
  return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
  return _compile(tmp_path_factory.mktemp("telemetry"), "telemetry", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
  """The same program with AddressSanitizer and UBSan: a program of its own, never loaded into Python."""
  return _compile(tmp_path_factory.mktemp("telemetry_san"), "telemetry_san",
                  ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _hex64(a):
  return " ".join(f"{int(w):x}" for w in np.ascontiguousarray(a, dtype=np.float64).ravel().view(np.uint64))


def _script(tel, B, ops):
  """The program's input and the twin's tables for a list of ("s", zm) / ("c", mask) / ("p",) ops."""
  Z = tel.n_zones
  twin = TelemetryTwin(tel, B)
  trace_of, first_row = tel.per_building(B)
  lines = [f"{B} {Z} {tel.n_traces} {tel.n_rows} {int(tel.per_zone)}", _hex64(tel.zone_temps),
           " ".join(str(int(k)) for k in trace_of), " ".join(str(int(k)) for k in first_row), _hex64(twin.weights)]
  want = []
  for op in ops:
    if op[0] == "s":
      lines.append("s " + _hex64(op[1]))
      twin.step(op[1])
    elif op[0] == "c":
      lines.append("c " + " ".join(str(int(m)) for m in op[1]))
      twin.close(op[1])
    else:
      lines.append("p")
      parts = [twin.running.ravel().view(np.uint64), twin.completed.ravel().view(np.uint64)]
      if tel.per_zone:
        parts += [twin.zone_running.ravel().view(np.uint64), twin.zone_completed.ravel().view(np.uint64)]
      parts.append(twin.action_rows().astype(np.uint64))
      want.append(np.concatenate(parts))
  return "\n".join(lines) + "\n", np.concatenate(want), twin


def _run(exe, text):
  out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
  return np.array([int(x, 16) for x in out], dtype=np.uint64)


def _traces(rng, n_traces, n_rows, Z, p_nan=0.2):
  t = rng.uniform(285.0, 305.0, size=(n_traces, n_rows, Z))
  t[rng.rand(*t.shape) < p_nan] = np.nan
  return t


@pytest.mark.parametrize("Z", [1, 2, 9])
def test_the_host_build_equals_the_twin_on_random_rows(program, Z):
  rng = np.random.RandomState(31 + Z)
  B, NT, NR = 6, 3, 8
  tel = Telemetry(_traces(rng, NT, NR, Z), trace_of=rng.randint(0, NT, size=B), first_row=rng.randint(0, NR, size=B),
                  zone_weights=rng.uniform(0.0, 3.0, size=Z), per_zone=True)
  ops = [("p",)]
  for t in range(11):                                                  # 11 steps on 8 rows: every building overruns
    ops += [("s", rng.uniform(285.0, 305.0, size=(B, Z))), ("p",)]
    if t in (3, 6):
      ops += [("c", rng.rand(B) < 0.5), ("p",)]
  text, want, twin = _script(tel, B, ops)
  assert np.array_equal(_run(program, text), want)
  assert (twin.completed[:, COL["steps"]] > 0).any() and (twin.running[:, COL["episode"]] > 0).any()
  assert (twin.running[:, COL["missing"]] >= Z).any() and (twin.running[:, COL["samples"]] > 0).any()
  assert (twin.zone_running[:, :, 0].sum(axis=1) == twin.running[:, COL["samples"]]).all()


def _edge_cases():
  """(name, telemetry, B, ops): the edges the issue lists, shared by the plain and the sanitized program."""
  rng = np.random.RandomState(9)
  Z, NR = 2, 4
  cases = []
  # NaN samples and an all-NaN row; zone weights that include 0
  t = rng.uniform(290.0, 300.0, size=(1, NR, Z))
  t[0, 1, 0] = np.nan
  t[0, 2, :] = np.nan
  tel = Telemetry(t, zone_weights=[0.0, 2.5], per_zone=True)
  steps = [("s", rng.uniform(290.0, 300.0, size=(2, Z))) for _ in range(NR)]
  cases.append(("nan", tel, 2, [x for s in steps for x in (s, ("p",))]))
  # first_row at the last row, then the overrun: one step reads the last row, the following ones nothing
  tel = Telemetry(t[:, :, :], first_row=[NR - 1, 0, NR - 1], per_zone=True)
  steps = [("s", rng.uniform(290.0, 300.0, size=(3, Z))) for _ in range(NR + 3)]
  cases.append(("last_row_and_overrun", tel, 3, [("p",)] + [x for s in steps for x in (s, ("p",))]))
  # a close before any step, two closes in a row
  tel = Telemetry(rng.uniform(290.0, 300.0, size=(NR, Z)), per_zone=True)
  one = np.ones(2, dtype=bool)
  cases.append(("closes", tel, 2, [("p",), ("c", one), ("p",), ("s", rng.uniform(290.0, 300.0, size=(2, Z))), ("p",),
                                   ("c", np.array([True, False])), ("p",), ("c", one), ("p",), ("c", one), ("p",)]))
  # a tie in max_abs_err: the same |e| at (row 0, zone 1) and again later -- the first occurrence stays
  rec = np.full((3, Z), 295.0)
  sims = [np.array([[295.0, 297.0]]), np.array([[293.0, 295.0]]), np.array([[297.0, 293.0]])]
  cases.append(("tie", Telemetry(rec), 1, [x for s in sims for x in (("s", s), ("p",))]))
  return cases


EDGES = _edge_cases()


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_the_host_build_equals_the_twin_at_the_edges(program, case):
  name, tel, B, ops = case
  text, want, twin = _script(tel, B, ops)
  assert np.array_equal(_run(program, text), want)
  run, done = twin.running, twin.completed
  if name == "nan":
    assert run[:, COL["samples"]].tolist() == [5, 5] and run[:, COL["missing"]].tolist() == [3, 3]
    assert (run[:, COL["weight_sum"]] == 3 * 2.5).all()                # zone 0 weighs nothing, zone 1 has three samples
    assert (twin.zone_running[:, :, 0] == [[2, 3], [2, 3]]).all()
  elif name == "last_row_and_overrun":
    assert run[:, COL["steps"]].tolist() == [7, 7, 7]
    assert run[:, COL["samples"]].tolist() == [2, 5, 2]                # (rows 1 and 2 hold three NaNs)
    assert run[:, COL["missing"]].tolist() == [12, 9, 12] and (run[:, COL["max_abs_row"]] < 4).all()
    assert twin.action_rows().tolist() == [3, 3, 3]
  elif name == "closes":
    assert done[:, COL["episode"]].tolist() == [0, 0] and done[:, COL["steps"]].tolist() == [1, 1]
    assert run[:, COL["episode"]].tolist() == [1, 1] and (run[:, COL["steps"]] == 0).all()
    assert (run[:, 7:10] == -1).all() and (twin.zone_running == 0).all() and (twin.zone_completed[:, :, 0] == 1).all()
  else:
    assert run[0, COL["max_abs_err"]] == 2.0 and run[0, COL["max_abs_row"]] == 0 and run[0, COL["max_abs_zone"]] == 1


def test_a_close_before_any_step_moves_no_bit(program):
  name, tel, B, ops = EDGES[2]
  text, want, _ = _script(tel, B, ops[:3])
  got = _run(program, text)
  assert np.array_equal(got, want) and np.array_equal(got[:len(got) // 2], got[len(got) // 2:])


@pytest.mark.parametrize("case", [EDGES[1]], ids=[EDGES[1][0]])
def test_overrun_and_last_row_under_the_sanitizers(sanitized, case):
  """Every trace row is an allocation of its own in the program: a read past the last row, or past a row's Z values,
  stops it (-fno-sanitize-recover), and the outputs still equal the twin."""
  name, tel, B, ops = case
  text, want, _ = _script(tel, B, ops)
  assert np.array_equal(_run(sanitized, text), want)


def test_telemetry_refuses_what_it_cannot_score():
  rec = np.full((2, 5, 3), 295.0)
  ok = Telemetry(rec.astype(np.float32), trace_of=[0, 1, 1, 0], first_row=[0, 4, 2, 1], zone_weights=[1, 0, 2],
                 actions=np.zeros((2, 5, 2), dtype=np.float32))
  ok.check(4, 3, 2)
  assert ok.zone_temps.dtype == np.float64 and ok.n_traces == 2 and ok.n_rows == 5 and ok.n_zones == 3 and ok.n_actions == 2
  assert Telemetry(rec[0]).n_traces == 1                               # [n_rows, Z]: one trace
  with pytest.raises(ValueError, match="shape"):
    Telemetry(np.zeros(5))
  with pytest.raises(ValueError, match="float32 or float64"):
    Telemetry(np.zeros((5, 3), dtype=np.int32))
  with pytest.raises(ValueError, match="3 zones, the floor plan 9"):
    ok.check(4, 9, 2)
  with pytest.raises(ValueError, match="trace_of has 4 rows, the batch 5"):
    ok.check(5, 3, 2)
  with pytest.raises(ValueError, match="2 columns, the simulator 3"):
    ok.check(4, 3, 3)
  bad = rec.copy()
  bad[1, 3, 2] = -np.inf
  with pytest.raises(ValueError, match="trace 1 row 3 zone 2 is infinite"):
    Telemetry(bad)
  bad[1, 3, 2] = np.nan
  Telemetry(bad)                                                       # NaN: no sample
  with pytest.raises(ValueError, match="building 2: trace_of 2 is outside the 2 traces"):
    Telemetry(rec, trace_of=[0, 1, 2])
  with pytest.raises(ValueError, match="building 1: trace_of -1"):
    Telemetry(rec, trace_of=[0, -1])
  with pytest.raises(ValueError, match="building 0: first_row 5 is outside the 5 rows"):
    Telemetry(rec, first_row=[5, 0])
  with pytest.raises(ValueError, match="building 3: first_row -2"):
    Telemetry(rec, first_row=[0, 0, 0, -2])
  with pytest.raises(ValueError, match=r"zone_weights\[1\]"):
    Telemetry(rec, zone_weights=[1.0, -0.5, 1.0])
  with pytest.raises(ValueError, match=r"zone_weights\[2\]"):
    Telemetry(rec, zone_weights=[1.0, 0.5, np.nan])
  with pytest.raises(ValueError, match="zone_weights must have shape"):
    Telemetry(rec, zone_weights=[1.0, 1.0])
  with pytest.raises(ValueError, match="2 traces of 4 rows, zone_temps 2 of 5"):
    Telemetry(rec, actions=np.zeros((2, 4, 2), dtype=np.float32))
  with pytest.raises(ValueError, match="finite"):
    Telemetry(rec, actions=np.full((2, 5, 2), np.inf, dtype=np.float32))


def test_telemetry_with_episode_starts_is_refused_before_anything_is_built():
  from tests import convection_cases as cc
  es = host_inputs.EpisodeStarts(offsets=host_inputs.UniformInt(0, 3))
  with pytest.raises(ValueError, match="telemetry together with episode_starts"):
    BatchedEnvironment(cc._plan(cc.TINY), 2, telemetry=Telemetry(np.full((4, 1), 295.0)), episode_starts=es)
  with pytest.raises(ValueError, match="host_inputs.Telemetry"):
    BatchedEnvironment(cc._plan(cc.TINY), 2, telemetry=np.full((4, 1), 295.0))


def test_header_ffi_and_names_agree():
  header = open(os.path.join(ROOT, "include", "sbsim_amd.h")).read()
  assert re.search(r"#define SB_ABI_VERSION 8\b", header) and _ffi.SB_ABI_VERSION == 8   # additive entries: the version stays
  assert int(re.search(r"#define SB_TL_FIELDS (\d+)", header).group(1)) == F == 13 == len(NAMES) == len(set(NAMES))
  assert int(re.search(r"#define SB_TL_ZONE_FIELDS (\d+)", header).group(1)) == ZF == 4 == len(_ffi.TELEMETRY_ZONE_SCORE_NAMES)
  enum = re.search(r"typedef enum sb_telemetry_score \{(.*?)\} sb_telemetry_score;", header, re.S).group(1)
  pairs = re.findall(r"SB_TL_([A-Z_]+) = (\d+)", enum)
  assert [(n.lower(), int(i)) for n, i in pairs] == [(n, i) for i, n in enumerate(NAMES)]
  for i, n in enumerate(NAMES):                                        # the documented table carries the same names
    assert re.search(rf"^ \*\s+{i} {n}\b", header, re.M), n
  for name in _ffi.TELEMETRY_ENTRIES:
    assert re.search(rf"^int {name}\(", header, re.M), name
  assert set(_ffi.TELEMETRY_ENTRIES) == {"sb_telemetry_attach", "sb_telemetry_detach", "sb_telemetry_get", "sb_telemetry_set",
                                         "sb_telemetry_zone_get", "sb_telemetry_zone_set", "sb_telemetry_actions"} <= set(_ffi.EXPORTS)
  struct = re.search(r"typedef struct sb_telemetry \{(.*?)\} sb_telemetry;", header, re.S).group(1)
  fields = re.findall(r"\b(\w+)(?=[;,])", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
  assert fields == [n for n, _ in _ffi.Telemetry._fields_]
  assert BatchedSimulator.TELEMETRY_SCORE_NAMES is NAMES is host_inputs.TELEMETRY_SCORE_NAMES
  assert BatchedEnvironment.TELEMETRY_SCORE_NAMES is NAMES is MixedBatchedEnvironment.TELEMETRY_SCORE_NAMES
  for cls in (BatchedSimulator, BatchedEnvironment, MixedBatchedEnvironment):
    for reader in ("telemetry_scores", "completed_telemetry_scores", "telemetry_zone_scores", "completed_telemetry_zone_scores",
                   "telemetry_actions"):
      assert callable(getattr(cls, reader)), (cls, reader)
  assert callable(BatchedSimulator.telemetry_attach) and callable(BatchedSimulator.telemetry_detach) and callable(BatchedSimulator.telemetry_set)


def test_the_built_library_exports_the_group():
  lib = _ffi.load()
  for name in _ffi.TELEMETRY_ENTRIES:
    assert hasattr(lib, name) and _ffi.telemetry_entry(name) is not None, name
  assert lib.sb_telemetry_get(None, None, None, None) == -1 and b"null argument" in lib.sb_last_error()
  assert lib.sb_telemetry_zone_set(None, None, None, None) == -1 and lib.sb_telemetry_actions(None, None, None) == -1
  assert lib.sb_telemetry_attach(None, None) == -1 and lib.sb_telemetry_detach(None) == -1
