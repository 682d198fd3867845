"""CPU: every case of tests/convection_cases.py reaches what it names, on the restatement alone.

A green tests/test_convection_cases_gpu.py means something only if the cases really run the instantiation, the partner
branch, the list links and the hops they claim.  These are conditions on the cases, not measurements: if a seed does not
meet one, the seed changes, not the assertion."""
import numpy as np
import pytest

from tests import convection_cases as cc


def _group(*groups):
  return [n for n, c in cc.CASES.items() if c.group in groups]


def test_every_case_of_the_issue_is_there():
  c = cc.CASES
  hand = [c[n] for n in _group("handover")]
  assert {(x.p, x.distance) for x in hand} == {(1.0, 5), (0.5, 5), (0.7, 20), (1.0, -1)}
  assert all(x.cus == 1 and x.plan == cc.TINY for x in hand)
  forced = [c[n] for n in _group("q") if c[n].force_q and c[n].plan == "q256"]
  assert sorted(x.q for x in forced) == list(range(1, 9))
  natural = {n: max(len(z) for z in cc.zones(cc.floor_plan(c[n]))) for n in _group("q") if not c[n].force_q}
  assert {256, 257, 600, 2047} <= set(natural.values())
  for plan in ("sizes", "shapes", "quirks"):
    got = {(x.p, x.distance) for x in c.values() if x.group == "shapes" and x.plan == plan}
    assert got == {(p, d) for _, p, d in cc.SETTINGS}, plan
  assert {(p, d) for _, p, d in cc.SETTINGS} == {(1.0, 5), (0.7, 20), (0.5, -1), (1.0, -1)}
  pins = {(x.pin, x.orientation) for x in c.values() if x.group == "layout"}
  kernels = {(k, w) for (k, _, w), _ in pins}
  assert kernels == {(cc.hc.REG, 1), (cc.hc.REG_PAIR, 2), (cc.hc.ROLL, 1), (cc.hc.TWO, 1), (cc.hc.BAND, 2), (cc.hc.BAND, 3), (cc.hc.BAND, 4),
                     (cc.hc.LDS, 1)}
  assert ((cc.hc.LDS, 0, 1), "rows") in pins and ((cc.hc.LDS, 0, 1), "columns") in pins
  for lay in {n.rsplit("-", 1)[0] for n in _group("layout")}:
    ds = {x.distance for x in c.values() if x.group == "layout" and x.name.startswith(lay + "-d")}
    assert {5, 20} <= ds, lay
  assert any(x.calls == 3 for x in c.values()) and any(x.first_building + x.B == 2 ** 32 for x in c.values())


def test_the_plans_have_the_rooms_they_are_named_for():
  sizes = lambda name: [len(z) for z in cc.zones(cc._plan(name))]
  assert sizes("sizes") == [600, 64, 65, 1, 2, 3]
  assert sizes("q256") == [256, 77, 15, 2]
  assert sorted(sizes("q257")) == [24, 257]
  assert sizes("one2047") == [2047] and cc._plan("one2047").shape == (29, 95)
  assert sizes("one2048") == [2048] and cc.MAX_ROOM == 2047
  assert sizes(cc.TINY) == [45] * 4
  assert sorted(sizes("shapes")) == [116 + 3, 120, 132]
  fp = cc._plan("shapes")
  H, W = fp.shape
  # the L is no rectangle, and the corridor's zone is two... four pieces: its bounding box is mostly other things
  for z in cc.zones(fp):
    x, y = np.divmod(z, W)
    box = (x.max() - x.min() + 1) * (y.max() - y.min() + 1)
    assert (box == len(z)) == (len(z) == 132)
  # zone_quirks: one zone made of two rooms (a gap of walls and other rooms between its parts), a one-cell zone
  q = cc._plan("quirks")
  assert 1 in sizes("quirks")
  two = [z for z in cc.zones(q) if (np.diff(np.unique(z // q.shape[1])) > 1).any()]
  assert len(two) == 1
  # the inputs: distinct values wherever a room is, exterior space at AMBIENT
  g = cc.input_grids(fp, 3)
  room = fp.zone_label >= 0
  assert len(np.unique(g[:, room])) == 3 * room.sum() and (g[:, fp.exterior_space] == cc.AMBIENT).all()
  assert not (fp.exterior_space & room).any() and g[2, 5, 5] == 2 * H * W + 5 * W + 5


@pytest.mark.parametrize("name", list(cc.CASES))
def test_instantiation_and_branches(name):
  case = cc.CASES[name]
  fp = cc.floor_plan(case)
  assert case.branches == cc.branches(fp, case.p, case.distance)
  if case.branches == (cc.ALL,):
    assert case.q is None
    return
  assert 1 <= case.q <= 8
  if not case.force_q:
    biggest = max(len(z) for z in cc.zones(fp))
    assert case.q == -(-biggest // 256) == cc.natural_q(fp)
  assert cc.threads(fp, case.q) <= 512 and cc.threads(fp, case.q) % 64 == 0


def test_branches_and_sizes_the_table_covers():
  c = cc.CASES
  assert {b for x in c.values() for b in x.branches} == {cc.TABLE, cc.RANK, cc.BOX, cc.ALL}
  # both wide branches inside ONE launch (rooms on either side of (2R + 1)^2 = 81 cells: 64 and 65 below, 600 above)
  assert c["sizes-d20"].branches == (cc.BOX, cc.RANK) and c["shapes-d20"].branches == (cc.BOX,)
  assert c["sizes-d1000"].branches == (cc.RANK,) and c["handover-d20"].branches == (cc.RANK,)
  # the box branch and the by-rank branch with the handle transposed, the box branch on every layout with rooms of 81 cells
  assert c["pair-d20"].branches == (cc.BOX,) and c["lds-columns-d20"].branches == (cc.BOX,) and c["pair-d1000"].branches == (cc.RANK,)
  assert all(c[n].orientation == "columns" for n in ("pair-d20", "lds-columns-d20", "pair-d1000", "lds-columns-all"))
  # workgroup sizes: 64, 128, 192 and 256 lanes, with the last cell-per-lane slot full, partly filled and empty
  fp = cc._plan("q256")
  assert [cc.threads(fp, q) for q in range(1, 9)] == [256, 128, 128, 64, 64, 64, 64, 64]
  assert cc.threads(cc._plan("q257"), 2) == 192 and cc.threads(cc._plan("sizes"), 3) == 256
  assert cc.threads(cc._plan("sizes"), 4) == 192 and cc.threads(cc._plan("one2047"), 8) == 256
  assert cc.natural_q(cc._plan("one2047")) == 8 and cc.natural_q(cc._plan("q257")) == 2
  # what is refused: 2048 cells; 600 cells at one per lane
  assert cc.threads(cc._plan(cc.TOO_SMALL_Q[0]), cc.TOO_SMALL_Q[1]) > 512
  assert max(len(z) for z in cc.zones(cc._plan(cc.REFUSED_ROOM))) == cc.MAX_ROOM + 1


def test_handover_depth():
  """With one CU at most 32 single-wavefront workgroups of k_convect are resident and k_convect_all gets 8: every
  workgroup runs at least DEPTH buildings, and the last round is partly empty for every possible grid size."""
  for name in _group("handover"):
    case = cc.CASES[name]
    fp = cc.floor_plan(case)
    if case.q is None:
      grids = [cc.ALL_PER_CU]
    else:
      assert cc.threads(fp, case.q) == 64      # one wavefront: at most MAX_RESIDENT workgroups on a CU
      grids = range(1, cc.MAX_RESIDENT + 1)
    for g in grids:
      assert case.B // g >= cc.DEPTH, (name, g)
    assert case.B % cc.MAX_RESIDENT and case.B % cc.ALL_PER_CU    # partly empty last round at the grids that matter


@pytest.mark.parametrize("name", _group("handover", "calls"))
def test_swap_sequences_make_the_chase_work(name):
  """From ConvectionOracle.swaps: some building and room has a cell chosen by >= 3 swaps (a list link is followed), a
  value moved by >= 3 successive swaps (the chase takes several hops) and a cell that starts no swap but is chosen by one;
  with p < 1 both included and excluded cells occur."""
  case = cc.CASES[name]
  if case.q is None:
    exp = cc.expected(case)[0]   # (the whole-room shuffle has no swaps) every building a permutation of its own
    room = (cc.floor_plan(case).zone_label >= 0).reshape(-1)
    moves = exp.reshape(case.B, -1)[:, room] - (np.arange(case.B) * exp[0].size)[:, None]
    assert len({m.tobytes() for m in moves}) == case.B
    return
  o = cc.oracle(case)
  chosen = hops = 0
  orphan = False
  started, cells = 0, 0
  for b in range(min(case.B, 24)):
    for z, zc in enumerate(o.zones):
      seq = o.swaps(b, z, 0)
      c, h, orph = cc.chase(len(zc), seq)
      chosen, hops, orphan = max(chosen, c), max(hops, h), orphan or orph
      started += len(seq)
      cells += len(zc)
  assert chosen >= 3 and hops >= 3 and orphan, (chosen, hops, orphan)
  if case.p < 1.0:
    # a cell starts no swap when it is excluded or picks itself: far fewer swaps than cells, yet many
    assert 0.2 * cells < started < 0.9 * cells, (started, cells)
    o1 = cc.oracle(cc.dataclasses.replace(case, p=1.0))
    assert sum(len(o1.swaps(0, z, 0)) for z in range(len(o1.zones))) > sum(len(o.swaps(0, z, 0)) for z in range(len(o.zones)))


def test_short_partner_lists():
  """(d): a cell whose partner list is itself alone -- in a room of one cell, and inside a zone of 119 cells (the
  one-cell closet of the corridor's zone); lists of two (the two-cell closet) and three cells (the corridor's dead end)."""
  for plan, big in (("sizes", 1), ("shapes", 119), ("quirks", 1)):
    counts = cc.partner_counts(cc._plan(plan), 5)
    assert any((n == 1).any() and len(n) == big for n in counts), plan
  shapes = [n for n in cc.partner_counts(cc._plan("shapes"), 5) if len(n) == 119][0]
  assert {1, 2, 3} <= set(shapes.tolist()) and shapes.max() == 21
  # the L's inner corner, the plan's edges: lists of every length in between
  assert len({int(v) for n in cc.partner_counts(cc._plan("shapes"), 5) for v in n}) >= 12
  # 2047 cells: a partner's list index needs all of the unsigned short table's 11 bits
  assert max(len(z) for z in cc.zones(cc._plan("one2047"))) - 1 == 0x7fe


@pytest.mark.parametrize("name", list(cc.CASES))
def test_restatement_permutes_rooms_leaves_the_rest_and_does_not_depend_on_sharding(name):
  case = cc.CASES[name]
  fp = cc.floor_plan(case)
  start = cc.input_grids(fp, case.B)
  exp = cc.expected(case)
  assert len(exp) == case.calls
  outside = fp.zone_label < 0
  before = start
  seen = []
  for k, g in enumerate(exp):
    assert np.array_equal(g[:, outside], start[:, outside])                       # walls, exterior space, unzoned air
    for z in cc.zones(fp):
      a, b = g.reshape(case.B, -1)[:, z], start.reshape(case.B, -1)[:, z]
      assert np.array_equal(np.sort(a, axis=1), np.sort(b, axis=1))               # every room keeps its values
    assert not np.array_equal(g, before)                                          # and the call moved some
    for b in range(case.B):
      assert not np.array_equal(g[b], before[b]), (k, b)
    seen.append(g.tobytes())
    before = g
  assert len(set(seen)) == case.calls
  # in shards: the same answer (first call; the later ones differ by the call number alone)
  cut = case.B // 2
  parts = []
  for lo, hi in ((0, cut), (cut, case.B)):
    part = start[lo:hi].copy()
    cc.oracle(case, case.first_building + lo).apply(part)
    parts.append(part)
  assert np.array_equal(np.concatenate(parts), exp[0])


@pytest.mark.parametrize("name", _group("layout"))
def test_layout_pins(name):
  """sb_plan_info (host only): the planner picks the pinned kernel for the case's plan, orientation and switches."""
  case = cc.CASES[name]
  info = cc.plan_info(case)
  assert (info["kernel"], info["path"], info["waves_per_building"]) == case.pin, info
