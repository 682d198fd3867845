"""CPU side of the coefficient regimes (tests/regimes.py).

(1) The oracle against the reference at every regime: tests/golden/regimes.npz holds runs of the reference's own
    Simulator (oracle/gen_golden_regimes.py); oracle/sb_oracle.c on the same inputs must give EQUAL sweep counts and
    converged flags and, as in tests/test_oracle_golden.py, bit-equal float64 temperatures.
(2) The coefficient facts that give each regime its purpose, on the compiled table of R9, and k_sweep_two's condition
    for measure-free periods (every b >= 0, every row sum <= 1) on every table the GPU test hands a kernel.
(3) Per (kernel case, regime): sb_plan_info picks the case's SB1 instantiation whatever the materials, and
    sb_debug_plan_digest shows that the tables did change.
(4) The conditions tests/test_regimes_gpu.py needs of its inputs, on the oracle twins of exactly its batches: no sweep's
    max|delta| within a relative 1e-9 of the threshold (so EQUAL sweep counts are a fair demand of a kernel that
    reassociates), no zone mean within 1e-6 K of a thermostat threshold, zone means inside 280 .. 310 K with zones in
    HEAT and in COOL, and each regime's sweep-count behaviour."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import regimes as rg
from tests.golden_util import load, oracle_params
from tests.twins import oracle_plan_of, step_kwargs

REGIMES = list(rg.REGIMES)
PAIRS = [(c, r) for c in rg.CASES for r in REGIMES]
HEAT, COOL = 1, 2                           # thermostat modes (oracle/sb_oracle.c)


# ---------------------------------------------------------------- (1) the oracle against the reference
@pytest.mark.parametrize("name", REGIMES)
def test_oracle_equals_the_reference_at_the_regime(name):
  from sbsim_amd.floorplan import FloorPlan, Materials
  g, regime = load(rg.GOLDEN), rg.REGIMES[name]
  assert list(g["regimes"]) == REGIMES
  fp = rg.apply(FloorPlan.from_file_input(g["floor_plan"], Materials.sb1(), 10.0, 300.0), regime)
  oplan = oracle_plan_of(fp)
  prm = oracle_params(g[f"{name}/params_json"])
  cfg = rg.case_config(rg.CASES["reg32-15x23"], regime)
  assert (prm.dt, prm.conv_threshold, prm.iter_limit) == (regime.time_step_sec, regime.convergence_threshold, cfg.iteration_limit)
  assert (prm.vav_max_air_flow, prm.vav_max_water_flow) == (cfg.vav_max_air_flow_rate, cfg.vav_reheat_max_water_flow_rate)
  init = g[f"{name}/initial_grid"]
  assert np.array_equal(init, rg.golden_inputs(regime, fp.shape))
  ob = orc.OracleBuilding(oplan, prm, 0.0, reset_temps=init.reshape(-1))
  comfort = g[f"{name}/comfort"]
  for t in range(rg.GOLDEN_STEPS):
    out = ob.step(now_ts=regime.time_step_sec * t, t_amb_now=float(g["t_amb"]), h_conv=float(g[f"{name}/h_conv"]),
                  t_amb_next=float(g["t_amb"]), comfort_now=bool(comfort[t]),
                  comfort_prev=bool(comfort[t - 1]) if t else False, comfort_next=bool(comfort[t + 1]), occupancy=1.0,
                  e_price=1e-8, e_carbon=1e-8, g_price=1e-8, g_carbon=1e-8, action=None, observe=False)
    assert out["n_sweeps"] == int(g[f"{name}/n_sweeps"][t]), (t, out["n_sweeps"])
    assert int(out["converged"]) == int(g[f"{name}/converged"][t]), t
    assert np.array_equal(out["zone_temp_post"], g[f"{name}/zone_temp_post"][t]), t
    assert np.array_equal(out["zone_temp_pre"], g[f"{name}/zone_temp_pre"][t]), t
    assert np.array_equal(out["mode"], g[f"{name}/mode"][t]), t
    assert out["blr_return_temp"] == g[f"{name}/blr_return_temp"][t], t
    assert out["ahu_flow"] == g[f"{name}/ahu_flow"][t] and out["blr_flow"] == g[f"{name}/blr_flow"][t], t
  assert np.array_equal(ob.grid(), g[f"{name}/final_grid"])


def test_reference_runs_cover_the_stopping_rules_edges():
  """The fixture itself: a regime whose run ends steps at the limit unconverged, steps of <= 2 sweeps, a fall of >= 40."""
  g = load(rg.GOLDEN)
  n = {r: g[f"{r}/n_sweeps"] for r in REGIMES}
  assert (g["stiff/converged"] == 0).any() and (g["stiff/converged"] == 1).any()
  assert (n["stiff"][g["stiff/converged"] == 0] == rg.LIMITS[("stiff", rg.GOLDEN_PLAN)]).all()
  assert n["contrast"].min() <= 2 and (n["hour"][:-1] - n["hour"][1:]).max() >= 40


# ---------------------------------------------------------------- (2) the coefficient facts
def _facts(cp):
  co = cp.class_coef
  b, ap, gc, sc = co[:, :4], co[:, 4], co[:, 5], co[:, 6]
  return dict(classes=cp.n_classes, max_b=b.max(), min_b=b[b > 0].min(), max_sum=b.sum(axis=1).max(),
              max_ap=ap.max(), min_ap=ap[b.sum(axis=1) > 0].min(), max_sc=sc.max())


#          max b            max row sum          max ap            max sc           classes - SB1's
RANGES = {
    "sb1":      ((0.2499, 0.25),   (0.9998, 0.9999),    (0.10, 0.11),     (5.5e-4, 5.6e-4),  0),
    "physical": ((0.17, 0.19),     (0.70, 0.74),        (0.97, 0.98),     (0.5, 1.0),        1),
    "short":    ((0.08, 0.09),     (0.33, 0.35),        (0.99, 1.0),      (0.3, 0.4),        1),
    "coarse":   ((0.05, 0.07),     (0.22, 0.25),        (0.99, 1.0),      (0.2, 0.3),        1),
    "stiff":    ((0.249, 0.25),    (0.997, 0.998),      (0.99, 1.0),      (0.01, 0.02),      1),
    "hour":     ((0.2499, 0.25),     (0.99998, 1.0),      (0.009, 0.01),    (5.5e-4, 5.6e-4),  0),
    "second":   ((0.24, 0.245),    (0.96, 0.97),        (0.97, 0.98),     (5.3e-4, 5.4e-4),  0),
    "contrast": ((0.2499, 0.25),   (0.99998, 1.0),      (0.99999, 1.0),   (5.5e-5, 5.6e-5),  1),
}


@pytest.mark.parametrize("name", REGIMES)
def test_coefficient_facts_of_the_regime(name):
  """On R9's compiled table."""
  f = _facts(rg.compiled(rg.CASES["roll-R9"], rg.REGIMES[name]))
  sb1 = _facts(rg.compiled(rg.CASES["roll-R9"], rg.REGIMES["sb1"]))
  b, s, ap, sc, dcls = RANGES[name]
  assert b[0] <= f["max_b"] <= b[1] and s[0] <= f["max_sum"] <= s[1], f
  assert ap[0] <= f["max_ap"] <= ap[1] and sc[0] <= f["max_sc"] <= sc[1], f
  assert f["classes"] - sb1["classes"] == dcls and sb1["classes"] == 20, f
  # each row's purpose
  if name in ("short", "coarse"):
    assert f["max_b"] < 0.1 and f["max_ap"] > 0.99                      # small b with ap near 1
  if name == "hour":
    assert f["max_sum"] > 0.99998 and f["min_ap"] < 1e-5                 # row sums near 1 with ap near 0
  if name == "contrast":
    assert f["max_b"] / f["min_b"] > 5e5 and f["min_b"] < 5e-7           # ap near 1, b over six decades
  if name == "physical":
    assert f["max_sc"] > 1000.0 * sb1["max_sc"]                          # sc a thousand times SB1's
  if name == "stiff":
    assert f["min_ap"] < 3e-3                                            # both ends of ap in one table


@pytest.mark.parametrize("case,name", PAIRS)
def test_tables_allow_measure_free_periods(case, name):
  """Dev::two_skip's condition (sbsim_hip.hip) on the table the device gets: every b >= 0, every cell's four summed in
  its order to <= 1.  Also: ap, gc and sc >= 0."""
  co = rg.compiled(rg.CASES[case], rg.REGIMES[name]).class_coef
  assert (co[:, :7] >= 0.0).all()
  assert ((((co[:, 0] + co[:, 1]) + co[:, 2]) + co[:, 3]) <= 1.0).all()


# ---------------------------------------------------------------- (3) the planner's choice and its tables
_SB1_INFO = {}


def _sb1_info(c):
  if c.name not in _SB1_INFO:
    _SB1_INFO[c.name] = rg.plan_info_and_digest(c, rg.REGIMES["sb1"])
  return _SB1_INFO[c.name]


VALUE_FREE = (rg.hc.LDS, rg.hc.REG, rg.hc.REG_PAIR)   # kernels that read class_coef itself: the planner's tables hold indices only


@pytest.mark.parametrize("case,name", PAIRS)
def test_kernel_choice_does_not_depend_on_the_materials(case, name):
  """sb_plan_info reports the case's SB1 instantiation at every regime (rg.pin: but for the one plan that sits at
  k_sweep_roll's class capacity), and the tables did change: sb_debug_plan_digest differs from SB1's wherever the
  planner's tables hold coefficients (k_sweep_roll's tmul, the coefficient sets of k_sweep_two / k_sweep_band /
  k_sweep_stream).  k_sweep_lds and k_sweep_reg read class_coef itself: the planner hands k_sweep_reg class indices only
  (its digest moves with the class structure alone) and k_sweep_lds the launch geometry; there class_coef is what must
  differ."""
  c, regime = rg.CASES[case], rg.REGIMES[name]
  info, digest = rg.plan_info_and_digest(c, regime)
  assert (info["kernel"], info["waves_per_building"], info["sweep_steps"], info["path"]) == rg.pin(c, regime)
  base, base_digest = _sb1_info(c)
  if rg.pin(c, regime) == (c.kernel, c.waves, c.steps, c.path):
    assert all(info[k] == base[k] for k in ("kernel", "path", "waves_per_building", "waves_per_workgroup", "sweep_steps"))
  if name == "sb1":
    assert digest == base_digest
    return
  cp, cp1 = rg.compiled(c, regime), rg.compiled(c, rg.REGIMES["sb1"])
  assert cp.class_coef.shape != cp1.class_coef.shape or not np.array_equal(cp.class_coef, cp1.class_coef)
  if info["kernel"] == rg.hc.LDS and base["kernel"] == rg.hc.LDS:
    assert digest == base_digest                        # the launch geometry alone
  elif info["kernel"] in VALUE_FREE:
    assert (digest == base_digest) == (cp.n_classes == cp1.n_classes and np.array_equal(cp.cell_class, cp1.cell_class)
                                       and info["kernel"] == base["kernel"])
  else:
    assert digest != base_digest


def test_one_plan_sits_at_the_roll_kernels_class_capacity():
  """rg.pin's exception, spelled out: 31 classes at the 20-class regimes, 32 at the others, and no other case moves."""
  c = rg.CASES["roll-47x48"]
  n = {r: rg.compiled(c, rg.REGIMES[r]).n_classes for r in REGIMES}
  assert n["sb1"] == rg.ROLL_CAPACITY and set(n.values()) == {rg.ROLL_CAPACITY, rg.ROLL_CAPACITY + 1}
  moved = [(k, r) for k in rg.CASES for r in REGIMES if rg.pin(rg.CASES[k], rg.REGIMES[r]) != rg.pin(rg.CASES[k], rg.REGIMES["sb1"])]
  assert moved == [("roll-47x48", r) for r in REGIMES if n[r] > rg.ROLL_CAPACITY] and 0 < len(moved) < len(REGIMES)


# ---------------------------------------------------------------- (4) the batches, on the oracle alone
def _counts(outs):
  n = np.array([[o["n_sweeps"] for o in row] for row in outs])
  conv = np.array([[int(o["converged"]) for o in row] for row in outs])
  return n, conv


@pytest.mark.parametrize("case,name", PAIRS)
def test_batch_conditions_on_the_oracle(case, name):
  c, regime = rg.CASES[case], rg.REGIMES[name]
  g = load("h2_sb1_r9_random.npz")
  cfg = rg.case_config(c, regime)
  outs = rg.oracle_rollout(c, regime)
  theta = cfg.convergence_threshold
  modes = set()
  for t, row in enumerate(outs):
    hsp, csp = rg.setpoints(g, t, cfg)
    for b, o in enumerate(row):
      assert (np.abs(o["max_delta"] - theta) > 1e-9 * theta).all(), (t, b)
      for tz in (o["zone_temp_pre"], o["zone_temp_post"], o["zone_air_temp"]):
        for edge in (hsp, csp, 0.5 * (csp - hsp) + hsp):
          assert np.abs(tz - edge).min() >= 1e-6, (t, b, edge)
        assert 280.0 < tz.min() and tz.max() < 310.0, (t, b, tz.min(), tz.max())
      modes |= set(o["mode"].tolist())
  assert {HEAT, COOL} <= modes
  n, conv = _counts(outs)
  limit = cfg.iteration_limit
  assert n.max() <= limit and (conv[n < limit] == 1).all()
  if name == "stiff":
    assert ((n == limit) & (conv == 0)).any() and ((n == limit) & (conv == 1)).any()
    assert ((n > 2) & (n < limit) & (conv == 1)).any()
  else:
    assert limit == regime.iteration_limit and (conv == 1).all()
  if name in ("contrast", "coarse"):
    assert (n <= 2).any()
  if name == "hour":
    assert (n[:-1] - n[1:]).max() >= 40                 # one building, from one step to the next
  if name == "second":
    assert n[1:].max() > 2 * n[0].max()                 # counts that rise after the first step


def test_mixed_materials_batch_conditions_on_the_oracle():
  """The batch of test_one_batch_carries_four_regimes_on_the_materials_handle: the same two distances, zone means inside
  280 .. 310 K, and buildings that differ."""
  g = load("h2_sb1_r9_random.npz")
  fp, cfg, ids, mats, hs, init, acts = rg.mixed_batch()
  assert mats[:, :, 0].max() / mats[:, :, 0].min() >= 1e6        # conductivities over six decades in one launch
  assert set(hs.tolist()) == {rg.REGIMES[r].h_conv for r in rg.MIXED}
  assert {(rg.REGIMES[r].time_step_sec, rg.REGIMES[r].cv_size_cm) for r in rg.MIXED} == {(cfg.time_step_sec, cfg.cv_size_cm)}
  twins = rg.mixed_twins(fp, cfg, ids, mats, init)
  theta, counts = cfg.convergence_threshold, set()
  for t in range(rg.MIXED_T):
    hsp, csp = rg.setpoints(g, t, cfg)
    for b in range(rg.MIXED_B):
      o = twins[b].step(**step_kwargs(g, rg.tc.TT0 + t, t, cfg, acts[t, b], h_conv=hs[b]), trace=True)
      assert (np.abs(o["max_delta"] - theta) > 1e-9 * theta).all(), (t, b)
      for tz in (o["zone_temp_pre"], o["zone_temp_post"], o["zone_air_temp"]):
        for edge in (hsp, csp, 0.5 * (csp - hsp) + hsp):
          assert np.abs(tz - edge).min() >= 1e-6, (t, b, edge)
        assert 280.0 < tz.min() and tz.max() < 310.0, (t, b, tz.min(), tz.max())
      counts.add(o["n_sweeps"])
  assert len(counts) >= 4


@pytest.mark.parametrize("name", REGIMES)
def test_jacobi_plans_qualify_at_the_regime(name):
  """The plans of test_jacobi_float32_class_tensors_at_every_regime pass solver="jacobi_fp32"'s checks, and the float32
  class tensors differ from SB1's."""
  from sbsim_amd.floorplan import jacobi_cv_tensors
  from tests import zone_ladder as zl
  r = rg.REGIMES[name]
  for kind, (_, nw) in zl.JACOBI.items():
    fp = rg.apply(zl.jacobi_plan(nw), r)
    assert fp.n_zones == nw
    t = jacobi_cv_tensors(fp, r.time_step_sec, r.h_conv)
    t1 = jacobi_cv_tensors(zl.jacobi_plan(nw), 300.0, 100.0)
    same = all(np.array_equal(np.asarray(t[k]), np.asarray(t1[k])) for k in t1)
    assert same == (name == "sb1")
