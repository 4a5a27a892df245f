"""CPU check that the sub-range comparison of tests/test_gpu_move_forms.py can fail: two oracle engines on its 37-character scene,
one following the range plan, the other making — once, in the first cycle after landing — one of the mistakes a broken move stage
would make (a sub-range shifted by one character; a character in two ranges of the same cycle). compare_states must tell them
apart at the first comparison and still at the last one of the run the GPU test makes, and must pass two engines that follow the
same plan. The list invariants the GPU tests hold the device's lists to (move_forms.check_schedule) are shown wrong lists as well.
Nothing of the product runs here."""
import pytest

import move_forms as mf
import oracle_binding as ob
from scenes import compare_states

SHIFTED = tuple((4, 5) if r == (3, 5) else r for r in mf.RANGE_PLAN)          # character 3 skipped, character 8 stepped instead
DOUBLED = tuple((15, 22) if r == (16, 21) else r for r in mf.RANGE_PLAN)      # character 15 stepped by (0, 16) and again by (15, 22)
CYCLES = 2 * mf.RANGE_CYCLES                                                  # the GPU case: RANGE_CYCLES under each of two thresholds


def _landed_engine(sge):
    eng = ob.oracle_engine()
    mf.scene(sge, eng, mf.RANGE_CROWD, 137)
    for _ in range(mf.LAND):
        mf.step(sge, eng)
    return eng


@pytest.fixture(scope="module")
def reference_run(sge):
    """The engine that follows the plan, stopped after every cycle: its states are what the others are compared with."""
    eng = _landed_engine(sge)
    assert mf.landed(sge, eng) > 0.8
    yield eng
    eng.close()


class _Frozen:
    """A downloaded state with the two methods compare_states reads."""

    def __init__(self, eng):
        self.state, self.pal = eng.download(), eng.palettes()

    def download(self):
        return self.state

    def palettes(self):
        return self.pal


@pytest.fixture(scope="module")
def reference_states(sge, reference_run):
    states = []
    for _ in range(CYCLES):
        mf.run_range_cycle(sge, reference_run)
        states.append(_Frozen(reference_run))
    return states


def test_two_engines_on_the_same_plan_agree(sge, reference_states):
    twin = _landed_engine(sge)
    for c in range(CYCLES):
        mf.run_range_cycle(sge, twin)
        compare_states(sge, twin, reference_states[c], mf.RANGE_CROWD)
    twin.close()


@pytest.mark.parametrize("wrong", [SHIFTED, DOUBLED], ids=["range_shifted_by_one", "character_in_two_ranges"])
def test_one_wrong_range_is_seen_at_once_and_to_the_end(sge, reference_states, wrong):
    bad = _landed_engine(sge)
    compared = []
    for c in range(CYCLES):
        mf.run_range_cycle(sge, bad, wrong if c == 0 else mf.RANGE_PLAN)
        if c in (0, mf.RANGE_CYCLES - 1, CYCLES - 1):
            with pytest.raises(AssertionError):
                compare_states(sge, bad, reference_states[c], mf.RANGE_CROWD)
            compared.append(c)
    assert compared == [0, mf.RANGE_CYCLES - 1, CYCLES - 1]
    bad.close()


def _schedule(cost, threshold, cap, first=0):
    """What correct list builders leave for `cost` (classify_kernel's rule, any order inside a class)."""
    import numpy as np
    cost = np.asarray(cost, np.int32)
    ids = np.arange(first, first + cost.size, dtype=np.int32)
    asking = ids[cost > threshold] if threshold >= 0 else ids[:0]
    heavy = asking[:cap]
    rest = np.setdiff1d(ids, heavy)
    order = rest[np.argsort(-mf.cost_class(cost[rest - first]), kind="stable")].astype(np.int32)
    counts = np.array([order.size, heavy.size, asking.size, int(np.maximum(cost, 0).sum())], np.int32)
    return {"counts": counts, "order": order, "heavy": heavy, "cost": cost, "cap": cap, "threshold": threshold, "built_for_next": True}


def test_the_list_invariants_can_fail():
    """check_schedule passes what correct builders leave and refuses each way the lists can be wrong: a character twice, a character
    missing, the order list rising in cost class, a heavy-listed character under the threshold, a list longer than the cap, counts
    that do not add up — on a 9-character sub-range that starts at 8, with a cut heavy list."""
    import numpy as np
    cost = np.array([900, 10, 300, 2000, 0, 129, 128, 127, 5000], np.int32)
    good = _schedule(cost, 200, 2, first=8)
    assert good["heavy"].size == 2 and good["counts"][2] == 4 and good["order"].size == 7
    mf.check_schedule(good, 8, 9, 200, None)
    mf.check_schedule(_schedule(cost, -1, 2, first=8), 8, 9, -1, None)
    mf.check_schedule(dict(good, built_for_next=False, cost=cost * 0), 8, 9, 200, cost)     # lists made from the step before

    def wrong(**kw):
        with pytest.raises(AssertionError):
            mf.check_schedule(dict(good, **kw), 8, 9, 200, None)

    twice = good["order"].copy()
    twice[3] = good["heavy"][0]                                            # stepped by both launches, and somebody skipped
    wrong(order=twice)
    wrong(order=good["order"][:-1], counts=good["counts"] - np.array([1, 0, 0, 0], np.int32))                # one character nowhere
    wrong(order=good["order"][::-1].copy())                                # cheapest class first
    cheap = int(good["order"][-1])
    wrong(heavy=np.array([good["heavy"][0], cheap], np.int32), order=np.append(good["order"][:-1], good["heavy"][1]).astype(np.int32))
    wrong(cap=1)                                                           # two listed where one fits
    wrong(counts=good["counts"] + np.array([0, 0, 1, 0], np.int32))        # a demand nobody asked for
    wrong(threshold=0)                                                     # lists of another threshold
