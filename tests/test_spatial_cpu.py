"""No GPU: the restatement of sb_spatial (tests/spatial_restatement.py) against NumPy, sb_spatial_shape, the binding.

Bounds (none taken from the code under test):
  zone mean   |restatement - np.mean| <= 2 (n - 1) 2^-53 max|T| for a zone of n cells: the bound of recursive summation,
              (n - 1) u max|T| with u = 2^-53 for n terms of magnitude <= max|T| (any order of n - 1 additions is within
              it to first order; the division adds one rounding, covered by the slack of the first-order bound for these
              n), taken twice because np.mean's pairwise sum errs too.
  tile        the float64 mean of either side is within n u max|T| of the exact one, far below half a float32 ulp
              (2^-24 relative), so the two float32 results are the same or neighbours: at most one float32 ulp apart."""
import ctypes as C

import numpy as np
import pytest

from sbsim_amd import _ffi, build, host_inputs
from tests import convection_cases as cc
from tests import spatial_restatement as sr
from tests import threshold_cases as tc


def _temps(fp, B, seed):
  H, W = fp.shape
  rs = np.random.RandomState(seed)
  return 270.0 + 40.0 * rs.rand(B, H, W)


@pytest.mark.parametrize("plan", ["R9", "sizes", "shapes", "quirks"])
def test_zone_statistics_against_numpy(plan):
  fp = tc.floor_plan("R9") if plan == "R9" else cc.PLANS[plan]()
  zones = fp.zone_cell_lists()
  t = _temps(fp, 3, 7)
  got = sr.zone_stats(t, zones)
  flat = t.reshape(3, -1)
  for z, cells in enumerate(zones):
    x = flat[:, cells]
    assert np.array_equal(got[:, z, 0], np.min(x, axis=1)) and np.array_equal(got[:, z, 1], np.max(x, axis=1))
    n = len(cells)
    bound = 2.0 * (n - 1) * 2.0 ** -53 * np.abs(x).max()
    err = np.abs(got[:, z, 2] - np.mean(x, axis=1)).max()
    assert err <= bound, (plan, z, n, err, bound)
  sizes = sorted(len(c) for c in zones)
  if plan == "sizes":
    assert sizes == [1, 2, 3, 64, 65, 600]     # a lone lane, a full round, one cell into the second round, ten rounds


def test_wave_order_is_not_numpys_order_but_is_exact_on_integers():
  """The restatement really sums in wave order: on values whose every partial sum is exact it equals the integer sum,
  and the order shows on values chosen so that two orders round differently."""
  x = np.arange(1000, dtype=np.float64)[None, :]
  assert sr.wave_order_sum(x)[0] == 999 * 1000 / 2 == sr.sequential_sum(x)[0]
  y = np.zeros((1, 130))
  y[0, 0], y[0, 64], y[0, 128] = 1.0, 2.0 ** -53, 2.0 ** -53   # lane 0: (1 + 2^-53) + 2^-53 = 1 in sequence
  y[0, 1] = 2.0 ** -52
  assert sr.wave_order_sum(y)[0] == 1.0 + 2.0 ** -52     # the exact sum is 1 + 2^-51: lane 0's sequence lost both 2^-53


@pytest.mark.parametrize("pool", [(1, 1), (4, 4), (5, 7), (8, 8), (9, 8), (68, 98), (100, 200)])
def test_tiles_against_numpy(pool):
  fp = tc.floor_plan("R9")
  H, W = fp.shape
  assert (H, W) == (68, 98)
  t = _temps(fp, 2, 11)
  got = sr.pooled_map(t, pool)
  mh, mw = sr.map_shape(H, W, pool)
  assert got.shape == (2, mh, mw) and got.dtype == np.float32
  for i in range(mh):
    for j in range(mw):
      ys, xs = sr.tile_cells(H, W, pool, i, j)
      want = np.mean(t[:, ys, xs].reshape(2, -1), axis=1).astype(np.float32)
      ulp = np.spacing(np.maximum(np.abs(want), np.abs(got[:, i, j])))
      assert (np.abs(got[:, i, j].astype(np.float64) - want.astype(np.float64)) <= ulp).all(), (pool, i, j)
  if pool == (1, 1):
    assert np.array_equal(got, t.astype(np.float32))


def test_ragged_and_whole_tiles_agree():
  """The vectorised path for pools that divide the grid makes the additions of the tile-by-tile path."""
  t = _temps(tc.floor_plan("R9"), 2, 3)[:, :64, :96]
  fast = sr.pooled_map(t, (4, 4))
  slow = np.zeros_like(fast)
  for i in range(16):
    for j in range(24):
      slow[:, i, j] = (sr.sequential_sum(t[:, 4 * i:4 * i + 4, 4 * j:4 * j + 4].reshape(2, -1)) / 16.0).astype(np.float32)
  assert np.array_equal(fast, slow)


def _shape(H, W, ph, pw):
  build.build()
  mh, mw = C.c_int32(-7), C.c_int32(-7)
  rc = _ffi.spatial_entry("sb_spatial_shape")(H, W, ph, pw, C.byref(mh), C.byref(mw))
  return rc, (mh.value, mw.value)


def test_spatial_shape():
  for pool, want in (((1, 1), (68, 98)), ((4, 4), (17, 25)), ((5, 7), (14, 14)), ((68, 98), (1, 1))):
    assert _shape(68, 98, *pool) == (0, want) and sr.map_shape(68, 98, pool) == want
  for pool in ((69, 98), (68, 99), (1000, 1000), (2 ** 31 - 1, 2 ** 31 - 1)):
    assert _shape(68, 98, *pool) == (0, (1, 1))
  assert _shape(68, 98, 2 ** 31 - 1, 1) == (0, (1, 98))
  for pool in ((0, 4), (4, 0), (0, 0), (-1, 4), (4, -1)):
    rc, out = _shape(68, 98, *pool)
    assert rc == -1 and out == (-7, -7)      # SB_ERR_INVALID, outputs untouched
    assert b"pool_h and pool_w must be >= 1" in _ffi.load().sb_last_error()
  assert _shape(0, 98, 4, 4)[0] == -1 and _shape(68, 0, 4, 4)[0] == -1
  assert _ffi.spatial_entry("sb_spatial_shape")(68, 98, 4, 4, None, None) == -1


def test_spatial_entry_asks_for_a_rebuild_on_a_library_without_the_entries(monkeypatch):
  class Stub:   # a library of the same ABI version built before the entries existed
    def sb_reset(self):
      pass
  monkeypatch.setattr(_ffi, "_lib", Stub())
  for name in _ffi.SPATIAL_ENTRIES:
    with pytest.raises(_ffi.SbsimError, match=f"has no {name}: rebuild"):
      _ffi.spatial_entry(name)
  assert set(_ffi.SPATIAL_ENTRIES) == {"sb_spatial_shape", "sb_spatial_attach", "sb_spatial"} <= set(_ffi.EXPORTS)


def test_null_handle_is_refused_without_a_gpu():
  build.build()
  assert _ffi.spatial_entry("sb_spatial_attach")(None, 4, 4, 0) == -1
  assert _ffi.spatial_entry("sb_spatial")(None, None, 1, None, None, None) == -1
  assert b"null handle" in _ffi.load().sb_last_error()


def test_spatial_outputs_checks_its_arguments():
  s = host_inputs.SpatialOutputs(pool=(4, 4))
  assert s.pool == (4, 4) and s.zone_stats and s == host_inputs.SpatialOutputs([4, 4], True)
  assert host_inputs.SpatialOutputs().pool is None
  assert host_inputs.SpatialOutputs(pool=(np.int64(2), 3), zone_stats=False).pool == (2, 3)
  for bad in ((0, 4), (4,), (4, 4, 4), (4.0, 4), "44", 4, (True, 4), (-1, 2), (2 ** 31, 1)):
    with pytest.raises(ValueError, match="pool must be"):
      host_inputs.SpatialOutputs(pool=bad)
  with pytest.raises(ValueError, match="asks for nothing"):
    host_inputs.SpatialOutputs(pool=None, zone_stats=False)
  with pytest.raises(ValueError, match="zone_stats must be a bool"):
    host_inputs.SpatialOutputs(zone_stats=1)
