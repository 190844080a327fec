"""Mixed-control steps (include/ccx.h: ccx_rollout_mixed), pinned to the reference on the CPU before any GPU is involved.

The contract is a composition of calls that exist: policy actions from the pre-step state, merged under the slot mask with
the caller's tensor, then the ordinary step.  Here the oracle computes that composition for every reference-recorded
mixed-control episode (tests/golden/mixed/, gen_golden_mixed.py: one side driven by the reference's own policy object, the
other by a seeded generator), with GARBAGE in the scripted slots of the tensor, and must reproduce the recording.  The
fixtures must also discriminate: without the mask the same tensor leaves the recording."""

import numpy as np
import pytest
from _fixtures import assert_step_matches
from _mixed import MIXED_NPZ, MixedGolden

from collectivecrossing_amd import configs as C
from collectivecrossing_amd.batched import scripted_slot_mask


def _c1(nb=5, ne=3):
    return C.CollectiveCrossingConfig(width=12, height=8, division_y=4, tram_door_left=5, tram_door_right=7, tram_length=9,
                                      num_boarding_agents=nb, num_exiting_agents=ne, exiting_destination_area_y=0,
                                      boarding_destination_area_y=8)


def test_scripted_slot_mask_accepts_every_documented_form():
    cfg = _c1()
    assert scripted_slot_mask(cfg, "boarding") == 0b00011111
    assert scripted_slot_mask(cfg, "exiting") == 0b11100000
    assert scripted_slot_mask(cfg, "all") == 0xFF
    assert scripted_slot_mask(cfg, [0, 7]) == 0b10000001
    assert scripted_slot_mask(cfg, (np.int64(2),)) == 0b100
    assert scripted_slot_mask(cfg, ["exiting_0", "boarding_1"]) == 0b00100010
    assert scripted_slot_mask(cfg, ["exiting_2", 0]) == 0b10000001
    assert scripted_slot_mask(cfg, "exiting_1") == 0b01000000
    assert scripted_slot_mask(cfg, iter([3])) == 0b1000
    assert scripted_slot_mask(cfg, 0b1010) == 0b1010 and scripted_slot_mask(cfg, np.uint64(5)) == 5
    assert scripted_slot_mask(cfg, 0) == 0 and scripted_slot_mask(cfg, []) == 0
    assert scripted_slot_mask(_c1(0, 3), "boarding") == 0 and scripted_slot_mask(_c1(0, 3), "exiting") == 0b111


@pytest.mark.parametrize("bad", ["exiting_3", "boarding_5", "nobody", [8], [-1], ["exiting_0", 9], 1 << 8, -1, [1.5], 2.0, True,
                                 [True]])
def test_scripted_slot_mask_refuses_unknown_ids_and_slots(bad):
    with pytest.raises(ValueError):
        scripted_slot_mask(_c1(), bad)


def test_the_recorded_episodes_cover_the_required_cases():
    gs = {n: MixedGolden(n) for n in MIXED_NPZ}
    assert len(gs) >= 6
    c1 = [g for g in gs.values() if g.N == 8 and g.params.num_boarding == 5]
    assert any(g.policy == "greedy" and g.mask == 0b11100000 for g in c1)          # C1, exiting scripted
    assert any(g.policy == "waiting" and g.mask == 0b00011111 for g in c1)         # C1, boarding scripted
    assert any(g.N == 32 for g in gs.values())                                     # C3 class
    assert any(g.N % 2 == 1 for g in gs.values())                                  # an odd agent count
    assert any(g.params.width == 100 and g.params.height == 100 for g in gs.values())   # the unfused path
    assert any(not g.identity_order() for g in gs.values())                        # shuffled dict order
    for g in gs.values():
        assert g["scripted_mask"].dtype == np.uint64 and g.policy in ("greedy", "waiting")


def _oracle_at_start(oracle, g):
    ob = oracle.OracleBatch(g.params, g.E)
    ob.set_state(**g.init_state())
    return ob


@pytest.mark.parametrize("name", MIXED_NPZ)
def test_the_oracle_composition_reproduces_the_reference(oracle, name):
    g = MixedGolden(name)
    tensor = g.tensor()
    ob = _oracle_at_start(oracle, g)
    sel = np.zeros(g.N, bool)
    sel[g.slots] = True
    for s in range(g.K):
        pa = ob.policy_actions(g.policy)
        merged = np.where(sel[None, :], pa, tensor[s])
        np.testing.assert_array_equal(merged, g["actions"][s], err_msg=f"{name} step {s}: merged actions")
        obs, rew, af, ef = ob.step(merged, g["order"][s])
        state = {k: getattr(ob, k) for k in ("x", "y", "active", "terminated", "truncated", "step_count")}
        assert_step_matches(g, s, obs, rew, af, ef, state)


@pytest.mark.parametrize("name", MIXED_NPZ)
def test_the_fixtures_discriminate(oracle, name):
    """A condition on the FIXTURES: the garbage tensor without a mask leaves the recording, and at least half of the
    scripted agent-steps differ from the garbage byte in their slot (uniform garbage: 0.8 expected)."""
    g = MixedGolden(name)
    tensor = g.tensor()
    asked = g["actions"][:, :, g.slots] != 255
    differ = asked & (g["actions"][:, :, g.slots] != tensor[:, :, g.slots])
    assert asked.sum() > 0 and 2 * differ.sum() >= asked.sum(), (int(differ.sum()), int(asked.sum()))
    ob = _oracle_at_start(oracle, g)
    diverged = False
    for s in range(g.K):
        ob.step(tensor[s], g["order"][s], want_obs=False)
        if not (np.array_equal(ob.x, g["x"][s]) and np.array_equal(ob.y, g["y"][s])):
            diverged = True
            break
    assert diverged, f"{name}: the garbage bytes happen to reproduce the recording"
