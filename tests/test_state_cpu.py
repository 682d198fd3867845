"""CPU-only checks of the state-snapshot entries (sb_state_save / sb_state_load): struct layouts, argument checks that
need no device, and the refusals of EnvSnapshot.from_state_dict."""
import ctypes as C
import os
import subprocess
import tempfile
import textwrap

import pytest

from sbsim_amd import _ffi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_struct_layouts_match_header():
  src = textwrap.dedent("""
      #include <stdio.h>
      #include <stddef.h>
      #include "sbsim_amd.h"
      int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(sb_state_view), sizeof(sb_state_clock),
                       offsetof(sb_state_view, occ), offsetof(sb_state_clock, was_reset), SB_STATE_NUM_SCALARS);
                       return 0; }
  """)
  with tempfile.TemporaryDirectory() as d:
    c = os.path.join(d, "p.c")
    open(c, "w").write(src)
    exe = os.path.join(d, "p")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    vals = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
  assert vals == [C.sizeof(_ffi.StateView), C.sizeof(_ffi.StateClock), _ffi.StateView.occ.offset,
                  _ffi.StateClock.was_reset.offset, _ffi.SB_STATE_NUM_SCALARS]


def test_state_entries_refuse_a_null_handle_or_view():
  build.build()
  L = _ffi.load()
  view, clk = _ffi.StateView(), _ffi.StateClock()
  view.n = 1
  assert L.sb_state_save(None, None, 1, C.byref(view), C.byref(clk), 0, None) == -1
  assert b"null handle" in L.sb_last_error()
  assert L.sb_state_save(None, None, 1, None, None, 0, None) == -1
  assert L.sb_state_load(None, None, C.byref(view), None, 0, None) == -1
  assert b"null handle" in L.sb_last_error()
  assert L.sb_state_load(None, None, None, C.byref(clk), 0, None) == -1


def test_missing_state_entries_ask_for_a_rebuild(monkeypatch):
  class Old:   # a library of the same ABI version built before the state entries
    pass
  monkeypatch.setattr(_ffi, "_lib", Old())
  with pytest.raises(_ffi.SbsimError, match="rebuild"):
    _ffi.state_entry("sb_state_save")


def test_env_snapshot_state_dict_needs_a_matching_fingerprint():
  torch = pytest.importorskip("torch")
  from sbsim_amd.environment import EnvSnapshot, SimState
  fp = ((68, 98, 9), "plan", "params", None, None)
  z = lambda *s: torch.zeros(s, dtype=torch.float64)
  i = lambda *s: torch.zeros(s, dtype=torch.int32)
  sim = SimState(z(2, 6), z(2, 4, 9), i(2, 9), z(2, 20), i(2), None, (0, 0, 0, 1), fp)
  snap = EnvSnapshot(sim, {"_step_count": 3}, None, {}, torch.zeros(2, 5), torch.zeros(2), None)
  d = snap.state_dict()
  back = EnvSnapshot.from_state_dict(d, "cpu")
  assert back.sim.fingerprint == fp and back.sim.clock == (0, 0, 0, 1) and back.host == {"_step_count": 3}
  missing = dict(d)
  del missing["fingerprint"]
  with pytest.raises(ValueError):
    EnvSnapshot.from_state_dict(missing, "cpu")
  other = dict(d, fingerprint=[(68, 98, 9), "another plan", "params", None, None])
  with pytest.raises(ValueError):
    EnvSnapshot.from_state_dict(other, "cpu")
  no_sim_fp = dict(d, sim={k: v for k, v in d["sim"].items() if k != "fingerprint"})
  with pytest.raises(ValueError):
    EnvSnapshot.from_state_dict(no_sim_fp, "cpu")
  with pytest.raises(ValueError):
    EnvSnapshot.from_state_dict({"grid": None}, "cpu")
