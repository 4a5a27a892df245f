"""GPU: every launch form and shortcut of pose_kernel against the float64 restatement of tests/pose_ref.py, at the rigs, profiles
and single-character rows of tests/pose_cases.py (what each rig reaches: pose_cases.RIGS and test_pose_reference.py::
test_pose_slot_contract). Pose stages only (locomotion, action, pose), uploaded state, three ticks (dt = 0, 1/64, 1/64), a tiny mesh,
the pose debug stores on. Per tick: the clocks against clocks_f64, the locals against locals_f64 of the DOWNLOADED post-tick state
with the families' bars (4 x the float32 oracle's measured worst), models and palettes against the staged float64 recomputation with
the derived bars, and the oracle's discrete state fields."""
import numpy as np
import pytest

import pose_cases as PC
import pose_ref as R

pytestmark = pytest.mark.gpu


def _check_tick(tag, rig, T, crowd, t, rows=slice(None)):
    sel = lambda d: {k: v[rows] for k, v in d.items()}
    clocks = R.clocks_f64(sel(t["before"]), t["dt"], rig.profiles)
    cw = R.check_clocks(sel(t["after"]), clocks, tag)
    ref = R.locals_f64(sel(t["after"]), T)
    worst, ratio = R.local_ratios(t["local"][rows], ref)
    print(f"{tag}: clocks {cw:.2f} locals " + " ".join(f"{f} {v:.1f}" for f, v in worst.items()), end=" ")
    bars = R.gpu_bars()
    for f, v in worst.items():
        if v > bars[f]:
            e, b = np.unravel_index(int(np.argmax(np.where(ref["family"] == R.FAMILIES.index(f), ratio, 0))), ratio.shape)
            raise AssertionError(f"{tag}: family {f} at {v:.1f} of its unit, bar {bars[f]:.1f}; worst: row {np.array(crowd['names'])[rows][e]!r} bone {b}")
    model, mbar = R.model_f64(t["local"][rows], rig.parent)
    mw = R.check_staged(t["model"][rows], model, mbar, tag + " model")
    pal, pbar = R.palette_f64(t["model"][rows], T.inv_bind.transpose(0, 2, 1).reshape(-1, 16))
    pw = R.check_staged(t["palette"][rows], pal, pbar, tag + " palette")
    print(f"| model {mw:.2f} palette {pw:.2f} of the derived bars")
    return worst, mw, pw


@pytest.mark.parametrize("name", list(PC.RIGS))
def test_pose_forms_against_float64(sge, name):
    rig, crowd, T, oracle_ticks = PC.oracle_case(sge, name)
    gpu = sge.CharacterEngine(0)
    try:
        ticks = list(PC.run_case(sge, gpu, rig, crowd))
    finally:
        gpu.close()
    for k, (t, o) in enumerate(zip(ticks, oracle_ticks)):
        _check_tick("%s tick %d" % (name, k), rig, T, crowd, t)
        for key in ("locomotion", "actions"):
            for f in ("state", "fromState", "flags"):
                if f in t["after"][key].dtype.names:
                    assert np.array_equal(t["after"][key][f], o["after"][key][f]), (name, k, key, f)
        assert t["after"]["bodies"].tobytes() == t["before"]["bodies"].tobytes()          # no move stage, no writeback


def test_sub_range_launch_leaves_the_others_alone(sge):
    """first = 3, count = 5 of 16 characters (the `first` offset of the launch): after a whole-crowd tick, two ticks of that range.
    Inside it everything is held as above; outside it the states and the palettes are byte-identical to before."""
    name = "b65_static_leaf"
    rig = PC.RIGS[name][0]()
    crowd = {k: v[4:20] for k, v in PC.rows(sge, rig).items()}
    first, count = 3, 5
    gpu = sge.CharacterEngine(0)
    try:
        ticks = list(PC.run_case(sge, gpu, rig, crowd, ticks=(PC.DT, PC.DT, 0.0), sub=(first, count)))
    finally:
        gpu.close()
    T = R.RigTables(rig, ticks[0]["built"])
    _check_tick("sub-range, whole crowd", rig, T, crowd, ticks[0])
    inside = slice(first, first + count)
    outside = np.r_[0:first, first + count:16]
    for k in (1, 2):
        _check_tick("sub-range tick %d" % k, rig, T, crowd, ticks[k], rows=inside)
        for key in ("locomotion", "actions", "bodies", "controllers"):
            assert ticks[k]["after"][key][outside].tobytes() == ticks[0]["after"][key][outside].tobytes(), (k, key)
        for what in ("palette", "model", "local"):
            assert ticks[k][what][outside].tobytes() == ticks[0][what][outside].tobytes(), (k, what)
    assert ticks[1]["palette"][inside].tobytes() != ticks[0]["palette"][inside].tobytes()
