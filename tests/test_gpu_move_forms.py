"""Every schedule of the move stage (csrc/sge_ccd.hip, launch_move) against the CPU oracle at the crowd sizes where the schedule
changes shape.

launch_move runs a step as move_kernel<0>, the list builders (classify / order_scan / order_scatter; the heavy list is cut at a cap
the host sizes from an older step's demand), the multi-wave move_kernel<1, *, true> over the heavy list, and move_group_kernel over
the order list (its leading min(128, count / 16) wavefronts take one character each) or, with SGE_MOVE_GROUP=0, the one-character
move_kernel<1, *>. All of it is "scheduling only": the CCD state must equal the oracle's bit for bit (scenes.compare_states)
whatever the lists say. A character stepped twice, skipped, or stepped by two launches is a wrong body, not a crash, so every case
here compares the whole crowd with the oracle, and every case reads the lists back from device memory
(CharacterEngine.move_schedule) to show which launches it reached: heavy list + order list hold every character of the ticked range
exactly once, the order list does not rise in cost class, nobody at or under the threshold is listed heavy, the heavy list is
min(cap, demand) long.

  sizes       2..9 (count & 7), 15 / 16 / 17 (count / 16 turns 1: the first solo wavefront), 31 / 33, 63 / 64 / 65 (a wavefront of
              the builders' lanes), 255 / 256 / 257 (a 256-thread block of the builders)
  thresholds  -1 (no multi-wave launch, lists built at the head of every stage), 0 (everybody who casts is heavy), and the median
              cost of the landed crowd (both lists populated, an order list shorter than the count)
  caps        SGE_HEAVY_CAP = 1, 3 (the cut) and 64 (>= count)
  ranges      the sub-range plan of tests/move_forms.py, back to back without host synchronisation
  switches    SGE_NO_SPEC (per tick), SGE_MOVE_GROUP=0 and SGE_MOVE_PIPELINE_LISTS=0 (per process: a child, move_forms_worker.py)

tests/test_move_forms_reference.py shows on the CPU that the sub-range comparison tells a wrong range from a right one."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import move_forms as mf
import oracle_binding as ob
from scenes import assert_struct_equal, compare_states

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65)
BLOCK_SIZES = (255, 256, 257)      # a shorter run after landing
AFTER, AFTER_BLOCK = 8, 4          # steps (= list generations) after landing
NO_SPLIT = (2, 3)                  # too few characters for a median that leaves somebody on either side for several steps


def _cases():
    out = []
    for n in SIZES + BLOCK_SIZES:
        for mode in ("-1", "0", "split"):
            if mode == "split" and n in NO_SPLIT:
                continue
            out.append(pytest.param(n, mode, False, id="n%d-thr%s" % (n, mode)))
    for n in (5, 17, 65):
        for mode in ("-1", "0", "split"):
            out.append(pytest.param(n, mode, True, id="n%d-thr%s-agents" % (n, mode)))
    return out


@pytest.fixture(scope="module")
def engines(sge):
    gpu = sge.CharacterEngine(0)
    cpu = ob.oracle_engine()
    yield gpu, cpu
    gpu.close()
    cpu.close()


def _exchange(sge, gpu, n, agents):
    if not agents:
        return None
    import torch
    return sge.parallel.AgentExchange(gpu, n, 0, 1, torch.device("cuda", 0), None)   # character-vs-character sweeps, world size 1


def _run(sge, gpu, cpu, n, mode, agents, after, seed, checks=None):
    """Lands the crowd and runs `after` further steps; mode "-1" / "0": that threshold from the first step on, "split": the default
    while landing, then the median cost. Compares with the oracle and checks the lists at `checks` and at every step after landing.
    Returns the threshold of the last steps and the schedule behind the last one."""
    A = sge.abi
    thr = mf.DEFAULT_THRESHOLD if mode == "split" else int(mode)
    gpu.set_option(A.OPT_HEAVY_THRESHOLD, thr)
    for e in (gpu, cpu):
        mf.scene(sge, e, n, seed, agents=agents)
    ex = _exchange(sge, gpu, n, agents)
    gpu.move_stats()
    total = mf.LAND + after
    checks = set(checks if checks is not None else (0, 1, 2, 12, 22, mf.LAND - 1)) | set(range(mf.LAND, total))
    sched = None
    for s in range(total):
        cost_before = gpu.move_cost() if s in checks else None
        for e in (gpu, cpu):
            mf.step(sge, e, exchange=ex)
        if s in checks:
            gpu.synchronize()
            compare_states(sge, gpu, cpu, n)
            sched = gpu.move_schedule()
            mf.check_schedule(sched, 0, n, thr, cost_before, tag="n=%d step %d" % (n, s))
            print("n=%d thr=%d step %d: order %d heavy %d demand %d cap %d for_next %d" % (
                n, thr, s, sched["counts"][0], sched["counts"][1], sched["counts"][2], sched["cap"], sched["built_for_next"]))
        if mode == "split" and s == mf.LAND - 1:
            thr = mf.split_threshold(sched["cost"])      # read through the accessor, from the landed crowd's last step
            gpu.set_option(A.OPT_HEAVY_THRESHOLD, thr)
    stats = gpu.move_stats()
    assert stats.overflow == 0 and stats.sweepTrips > 0
    assert mf.landed(sge, gpu) > 0.8, "most characters should have landed: before, costs are zero and every schedule is the same launch"
    return thr, sched


@pytest.mark.parametrize("n,mode,agents", _cases())
def test_edge_crowd_sizes_and_thresholds(sge, engines, n, mode, agents):
    gpu, cpu = engines
    thr, sched = _run(sge, gpu, cpu, n, mode, agents, AFTER_BLOCK if n in BLOCK_SIZES else AFTER, seed=100 + n)
    if mode == "split":
        assert sched["order"].size > 0 and sched["heavy"].size > 0, ("the threshold must split the crowd", thr, sched["cost"])
        assert sched["built_for_next"]
    elif mode == "0":
        assert sched["heavy"].size > 0.8 * n and sched["built_for_next"], sched["counts"]   # everybody who stands casts: the multi-wave launch
    else:
        assert sched["heavy"].size == 0 and sched["order"].size == n and not sched["built_for_next"]


@pytest.mark.parametrize("cap", [1, 3, 64])
def test_heavy_list_cut_at_the_cap(sge, monkeypatch, cap):
    """SGE_HEAVY_CAP (read when the context is created) cuts the heavy list: who does not fit stays with the grouped launch. 33
    characters, threshold 0: the demand is the whole landed crowd, so caps 1 and 3 cut and 64 does not (the multi-wave grid is then
    the count). Then the threshold changes 0 -> split -> -1 -> 0 with the previous step still in flight."""
    monkeypatch.setenv("SGE_HEAVY_CAP", str(cap))
    A = sge.abi
    n = 33
    gpu, cpu = sge.CharacterEngine(0), ob.oracle_engine()
    try:
        _, sched = _run(sge, gpu, cpu, n, "0", False, AFTER, seed=133)
        counts = sched["counts"]
        assert sched["cap"] <= cap and counts[1] == min(cap, counts[2]), (counts, sched["cap"])
        if cap < n:
            assert counts[2] > cap, ("the case must cut the list", counts)
            assert sched["order"].size == n - cap
        else:
            assert counts[1] == counts[2] > 0.8 * n
        split = mf.split_threshold(sched["cost"])
        for thr in (split, -1, 0):
            for e in (gpu, cpu):
                mf.step(sge, e)                              # in flight while the option changes
            gpu.set_option(A.OPT_HEAVY_THRESHOLD, thr)
            for _ in range(2):
                for e in (gpu, cpu):
                    mf.step(sge, e)
            cost_before = gpu.move_cost()
            for e in (gpu, cpu):
                mf.step(sge, e)
            gpu.synchronize()
            compare_states(sge, gpu, cpu, n)
            sched = gpu.move_schedule()
            mf.check_schedule(sched, 0, n, thr, cost_before, tag="cap %d thr %d" % (cap, thr))
            print("cap=%d thr=%d: counts %s cap %d" % (cap, thr, sched["counts"], sched["cap"]))
            assert sched["cap"] <= cap
            if thr == split:
                assert sched["counts"][2] > 0 and sched["order"].size > 0 and sched["heavy"].size > 0
        assert gpu.move_stats().overflow == 0
    finally:
        gpu.close()
        cpu.close()


def test_sub_range_move_stages_against_the_oracle(sge, engines):
    """The sub-range plan (lists + count, first + i and the heavy grid all depend on the range) under threshold 0 and under the
    splitting threshold, tick after tick without host synchronisation, every range handed identically to the oracle. The sibling
    of test_move_lists_are_rebuilt_behind_the_build_in_flight with the oracle as the reference."""
    gpu, cpu = engines
    A = sge.abi
    n = mf.RANGE_CROWD
    gpu.set_option(A.OPT_HEAVY_THRESHOLD, mf.DEFAULT_THRESHOLD)
    for e in (gpu, cpu):
        mf.scene(sge, e, n, 137)
    gpu.move_stats()
    for _ in range(mf.LAND):
        for e in (gpu, cpu):
            mf.step(sge, e)
    gpu.synchronize()
    compare_states(sge, gpu, cpu, n)
    assert mf.landed(sge, gpu) > 0.8
    sched = gpu.move_schedule()
    last_first, last_count = mf.RANGE_PLAN[-1]
    for thr in (0, mf.split_threshold(sched["cost"])):
        gpu.set_option(A.OPT_HEAVY_THRESHOLD, thr)
        for c in range(mf.RANGE_CYCLES):
            for e in (gpu, cpu):
                mf.run_range_cycle(sge, e)
            gpu.synchronize()
            compare_states(sge, gpu, cpu, n)
            part = gpu.move_schedule(last_first, last_count)
            assert part["built_for_next"]
            mf.check_schedule(part, last_first, last_count, thr, None, tag="thr %d cycle %d" % (thr, c))
            with pytest.raises(sge.SgeError):
                gpu.move_schedule(0, 0)              # not the newest stage's range: refused, not read from another range's layout
        for e in (gpu, cpu):
            mf.step(sge, e)
        gpu.synchronize()
        compare_states(sge, gpu, cpu, n)
        whole = gpu.move_schedule()
        mf.check_schedule(whole, 0, n, thr, None, tag="thr %d whole crowd" % thr)
        print("thr=%d: counts %s" % (thr, whole["counts"]))
        assert whole["heavy"].size > 0
    assert whole["order"].size > 0, "the second threshold must split the crowd"
    stats = gpu.move_stats()
    assert stats.overflow == 0 and stats.sweepTrips > 0


@pytest.mark.parametrize("n", [17, 65])
@pytest.mark.parametrize("mode", ["0", "split"])
def test_no_speculative_casts_same_result(sge, engines, monkeypatch, n, mode):
    """SGE_NO_SPEC (read on every tick) takes the speculative ground samples out of every launch form: same bits as the oracle, and
    the same bits as the speculative run of the same crowd."""
    gpu, cpu = engines
    _run(sge, gpu, cpu, n, mode, False, AFTER, seed=200 + n, checks=(mf.LAND - 1,))
    spec = gpu.download(what=("bodies", "controllers"))
    monkeypatch.setenv("SGE_NO_SPEC", "1")
    _run(sge, gpu, cpu, n, mode, False, AFTER, seed=200 + n)
    plain = gpu.download(what=("bodies", "controllers"))
    assert_struct_equal(plain["bodies"], spec["bodies"], "bodies without / with speculation", skip=())
    assert_struct_equal(plain["controllers"], spec["controllers"], "controllers without / with speculation", skip=())


class _Recorded:
    """One run of the child's .npz with the two methods compare_states reads."""

    def __init__(self, z, key):
        self.z, self.key = z, key

    def download(self):
        return {k: self.z[self.key + k] for k in ("bodies", "controllers", "locomotion", "actions")}

    def palettes(self):
        return self.z[self.key + "palettes"], None, None


# What the same crowds take in process (test_edge_crowd_sizes_and_thresholds, n = 17 and n = 65 under -1 and 0, oracle and
# comparisons included), measured on an MI355X: 0.07 s at n = 65 and less at n = 17, 0.3 s for the four runs together. The child does
# the GPU half of that; the 2.3 s it was measured to take are the interpreter, the imports and the context.
IN_PROCESS_SECONDS = 0.3
CHILD_TIMEOUT = 60.0 + 20.0 * IN_PROCESS_SECONDS      # a minute for start-up on a busy machine, twenty times the work


@pytest.mark.parametrize("switch", ["SGE_MOVE_GROUP", "SGE_MOVE_PIPELINE_LISTS"])
def test_process_wide_switches_in_a_child(sge, engines, tmp_path, switch):
    """SGE_MOVE_GROUP=0 (no grouped launch: the one-character move_kernel<1, *> that skips whoever is flagged heavy, no order list)
    and SGE_MOVE_PIPELINE_LISTS=0 (lists built at the head of every stage) are static in launch_move: each runs in a fresh child
    (n = 17 and n = 65 under thresholds -1 and 0 in one process) whose recorded state is compared with the oracle here.
    Time limit: the four in-process runs of these sizes and thresholds were measured at 0.3 s together on an MI355X (0.07 s at
    n = 65), the child at 2.3 s, nearly all of it start-up; it gets a minute for start-up plus twenty times the work (66 s)."""
    _, cpu = engines
    steps = mf.LAND + AFTER
    out = tmp_path / (switch + ".npz")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "move_forms_worker.py")
    cmd = [sys.executable, worker, "--sizes", "17,65", "--thresholds=-1,0", "--steps", str(steps), "--seed-base", "100", "--out", str(out)]
    t0 = time.time()
    try:
        done = subprocess.run(cmd, env=dict(os.environ, **{switch: "0"}), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        pytest.fail("%s=0: the child ran into its limit of %.0f s\n%s" % (switch, CHILD_TIMEOUT, e.stderr))
    print("%s=0: child took %.1f s" % (switch, time.time() - t0))
    assert done.returncode == 0, "%s=0: the child failed (%d)\n%s\n%s" % (switch, done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    z = np.load(str(out))
    for n in (17, 65):
        for thr in (-1, 0):
            key = "n%d_t%d_" % (n, thr)
            mf.scene(sge, cpu, n, 100 + n)
            for _ in range(steps):
                mf.step(sge, cpu)
            compare_states(sge, _Recorded(z, key), cpu, n)
            counts = z[key + "counts"]
            assert z[key + "overflow"] == 0 and z[key + "sweepTrips"] > 0
            # evidence that the switch arrived: no order list without the grouped launch; no lists built ahead without the pipeline
            if switch == "SGE_MOVE_GROUP":
                assert counts[0] == 0 and counts[1] == (0 if thr < 0 else counts[2]) and not z[key + "built_for_next"], (key, counts)
            else:
                assert counts[0] + counts[1] == n and not z[key + "built_for_next"], (key, counts)
            if thr == 0:
                assert counts[1] > 0.8 * n, (key, counts)
