"""NumPy replay of k_sweep_roll's schedule with free periods (test utility, CPU only): the rolling sweeps of
tests/kernel_model.py's RegSweepModel plus what step_roll.hip's library kernel adds to them -- the travelling
accumulators (struct Acc: `tr` moves one lane down per tracked step and carries one column of one sweep, lane 63
collects what leaves in `fin`), the proof at a period's top (max of `tr` over the lanes, high words, strictly above the
threshold's) and the two period bodies: a free period (plain steps untracked, window steps tracked, no copies) and a
measuring period (today's).  Next to the kernel's bookkeeping the model keeps every sweep's true max|delta| by lane
masks, which is what the hygiene assertions compare with."""
import numpy as np

from tests.kernel_model import RegSweepModel

K_WIN = 63


def hi32(x):
  """High words of non-negative doubles (order like the doubles)."""
  return (np.abs(np.asarray(x, dtype=np.float64)).view(np.uint64) >> np.uint64(32)).astype(np.int64)


class RollFreeModel(RegSweepModel):

  def fd_timestep_free(self, temp, t_amb, q_zone, thr, iter_limit, free=True):
    """-> (grid, sweeps, log); log: per period (kind, proof high word at its top, the sweep's true max|delta|)."""
    cp, NR = self.cp, self.NR
    assert self.mode in (1, 3) and NR > K_WIN
    full = np.array(temp, dtype=np.float64).reshape(cp.H, cp.W)
    ring_mask = np.ones((cp.H, cp.W), bool)
    ring_mask[self.x0:self.x1 + 1, self.y0:self.y1 + 1] = False
    ring = full[ring_mask]
    g = np.zeros(cp.n_classes + 1)
    g[:-1] = cp.class_coef[:, 5] * t_amb + cp.class_coef[:, 6] * np.where(
        cp.class_zone >= 0, q_zone[np.maximum(cp.class_zone, 0)], 0.0)
    es, tail = self._load(full[self.x0:self.x1 + 1, self.y0:self.y1 + 1])
    e, A = es[0], self._a_pass(es[0], 0, g)
    tcls = np.array([[self._class(np.array(64 + t), np.array(c)) for c in range(NR)] for t in range(self.T)],
                    dtype=np.int64).reshape(self.T, NR)
    At = self.coef[tcls, 4] * tail + g[tcls] if self.T else None
    ring_d = max(abs(t_amb - ring.min()), abs(t_amb - ring.max())) if ring.size else 0.0
    lane = np.arange(64)
    thr_hi = int(hi32(thr))
    log = []

    def step(D, first):
      r, rm, rp = D % NR, (D - 1) % NR, (D + 1) % NR
      col = (D - lane) if first else (D - lane) % NR
      co = self.coef[self._class(lane, col)]
      U = np.empty(64); U[1:] = e[:-1, rm]; U[0] = 0.0
      Dn = np.empty(64); Dn[:-1] = e[1:, rp]
      tc = col[63]
      Dn[63] = tail[0, tc] if (self.T and 0 <= tc < NR) else 0.0
      nv = co[:, 1] * Dn + A[:, r]
      nv = co[:, 3] * e[:, rp] + nv
      nv = co[:, 2] * e[:, rm] + nv
      nv = co[:, 0] * U + nv
      sel = np.where((lane <= D) if first else True, nv, e[:, r])
      d, old = np.abs(sel - e[:, r]), e[:, r].copy()
      e[:, r] = sel
      return d, old

    acc = dict(tr=np.zeros(64, dtype=np.int64), fin=0)

    def track(d):   # step_roll.hip track(): lane 63 collects what arrived with the previous step, then everything moves
      acc["fin"] = max(acc["fin"], int(acc["tr"][63]))
      moved = np.concatenate([[0], acc["tr"][:-1]])
      acc["tr"] = np.maximum(moved, hi32(d))

    def period_end():
      acc["fin"] = 0
      acc["tr"][63] = 0

    dcur = np.zeros(64)   # the model's own bookkeeping: max|delta| of the sweep in progress, per lane
    for D in range(K_WIN):
      d, _ = step(D, True)
      track(d)
      dcur = np.maximum(dcur, d)
    n = 0
    while True:
      # ---- the top test: tr of lanes 0..62 = partial maxima of columns 62 - l of the sweep in progress
      assert acc["tr"][63] == 0 and acc["fin"] == 0
      top = int(acc["tr"].max())
      if n == 0:
        top = max(top, int(hi32(ring_d)))
      is_free = free and top > thr_hi and n + 1 < iter_limit
      dnext, bk = np.zeros(64), []
      for D in range(K_WIN, NR):
        d, _ = step(D, False)
        if not is_free:
          track(d)
        dcur = np.maximum(dcur, d)
      for j in range(K_WIN):
        d, old = step(NR + j, False)
        track(d)
        if not is_free:
          bk.append(old)
        dcur = np.maximum(dcur, np.where(lane > j, d, 0.0))
        dnext = np.maximum(dnext, np.where(lane <= j, d, 0.0))
      md = float(dcur.max())
      dt = self._tail_pass(tail, At, tcls, e[63, (np.arange(NR) + 63) % NR].copy()) if self.T else 0.0
      md = max(md, dt, ring_d if n == 0 else 0.0)
      log.append(("free" if is_free else "measuring", top, md))
      if is_free:
        assert md > thr, "a free period finished a sweep that ends the step"
      else:
        acc["fin"] = max(acc["fin"], int(acc["tr"][63]))   # the period's last step
        m_hi = max(acc["fin"], int(hi32(dt)), int(hi32(ring_d)) if n == 0 else 0)
        # hygiene: whatever ran before, a measuring period sees its own sweep's 96 column maxima and nothing else
        assert m_hi == int(hi32(md)), (n, m_hi, int(hi32(md)))
      n += 1
      period_end()
      # lanes 0..62 hold the started sweep's partial maxima and nothing of the finished one
      assert (acc["tr"][:K_WIN] <= int(hi32(dnext.max()))).all() and int(acc["tr"].max()) == int(hi32(dnext.max()))
      if not is_free:
        assert m_hi != thr_hi, "the exact kernel's case: not modelled"
        if m_hi < thr_hi or n >= iter_limit:
          for j in range(K_WIN):
            e[:, j] = np.where(lane <= j, bk[j], e[:, j])
          break
      dcur = dnext
    out = full.copy()
    out[ring_mask] = t_amb
    out[self.x0:self.x1 + 1, self.y0:self.y1 + 1] = self._store([e], tail)
    return out, n, log
