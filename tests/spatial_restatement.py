"""NumPy restatement of sb_spatial (test utility, no GPU): zone {min, max, mean} and the pooled map of a [B, H, W] float64
array, in exactly the summation order include/sbsim_amd.h documents (SUMMATION ORDER):

  wave order of a list x[0..n):  lane l of 64 starts from +0.0 and adds x[l], x[l+64], ... in sequence; then for
      o = 32, 16, 8, 4, 2, 1 every lane takes s[l] + s[l xor o].  Min and max likewise from +inf / -inf.
  zone:  wave order of its cells in ascending flat index of the caller's grid (FloorPlan.zone_cell_lists());
         mean = sum / n.
  tile:  pool_h * pool_w <= 64 -- +0.0, then the tile's cells row-major in sequence; more -- wave order of the
         row-major list.  The mean (sum / count, float64) is stored as float32.

Every addition below is one IEEE float64 addition, as on the device (the library is built with -ffp-contract=off)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

LANES = 64
LANE_TILE = 64   # kSpatialLaneTile


def map_shape(H: int, W: int, pool: Tuple[int, int]) -> Tuple[int, int]:
  return (-(-H // pool[0]), -(-W // pool[1]))


def wave_order_sum(x: np.ndarray) -> np.ndarray:
  """x: [B, n] float64 -> [B] in wave order."""
  B, n = x.shape
  s = np.zeros((B, LANES), dtype=np.float64)
  for k in range(0, n, LANES):     # lane l adds x[l + k]: one addition per lane and round, in sequence
    w = min(LANES, n - k)
    s[:, :w] = s[:, :w] + x[:, k:k + w]
  lane = np.arange(LANES)
  o = LANES // 2
  while o:
    s = s + s[:, lane ^ o]
    o //= 2
  assert (s == s[:, :1]).all()     # every lane ends with the same bits
  return s[:, 0].copy()


def sequential_sum(x: np.ndarray) -> np.ndarray:
  """x: [B, n] -> [B]: +0.0, then x[0], x[1], ... added in sequence."""
  s = np.zeros(x.shape[0], dtype=np.float64)
  for k in range(x.shape[1]):
    s = s + x[:, k]
  return s


def zone_stats(temps: np.ndarray, zone_cells: Sequence[np.ndarray]) -> np.ndarray:
  """temps [B, H, W] float64, zone_cells: per zone the flat cell indices, ascending -> [B, Z, 3] {min, max, mean}."""
  B = temps.shape[0]
  flat = np.ascontiguousarray(temps, dtype=np.float64).reshape(B, -1)
  out = np.zeros((B, len(zone_cells), 3), dtype=np.float64)
  for z, cells in enumerate(zone_cells):
    cells = np.asarray(cells, dtype=np.int64)
    assert len(cells) and (np.diff(cells) > 0).all()
    x = flat[:, cells]
    out[:, z, 0] = x.min(axis=1)   # (min and max do not depend on the order)
    out[:, z, 1] = x.max(axis=1)
    out[:, z, 2] = wave_order_sum(x) / np.float64(len(cells))
  return out


def tile_cells(H: int, W: int, pool: Tuple[int, int], i: int, j: int) -> Tuple[slice, slice]:
  return (slice(i * pool[0], min((i + 1) * pool[0], H)), slice(j * pool[1], min((j + 1) * pool[1], W)))


def pooled_map(temps: np.ndarray, pool: Tuple[int, int]) -> np.ndarray:
  """temps [B, H, W] float64 -> [B, map_h, map_w] float32."""
  B, H, W = temps.shape
  mh, mw = map_shape(H, W, pool)
  t = np.ascontiguousarray(temps, dtype=np.float64)
  out = np.zeros((B, mh, mw), dtype=np.float32)
  wave = pool[0] * pool[1] > LANE_TILE
  if not wave and H % pool[0] == 0 and W % pool[1] == 0:   # no ragged tile: every tile at once, the same additions
    x = t.reshape(B, mh, pool[0], mw, pool[1]).transpose(0, 1, 3, 2, 4).reshape(B * mh * mw, pool[0] * pool[1])
    return (sequential_sum(x) / np.float64(pool[0] * pool[1])).astype(np.float32).reshape(B, mh, mw)
  for i in range(mh):
    for j in range(mw):
      ys, xs = tile_cells(H, W, pool, i, j)
      x = t[:, ys, xs].reshape(B, -1)
      s = wave_order_sum(x) if wave else sequential_sum(x)
      out[:, i, j] = (s / np.float64(x.shape[1])).astype(np.float32)
  return out


def spatial(temps: np.ndarray, zone_cells: Sequence[np.ndarray], pool: Optional[Tuple[int, int]],
            rows: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
  """(zone statistics, map or None) of buildings `rows` (None: all, in order)."""
  t = temps if rows is None else temps[np.asarray(rows, dtype=np.int64)]
  return zone_stats(t, zone_cells), None if pool is None else pooled_map(t, pool)
