"""CPU: the float32 oracle's pose stage against the float64 restatement of tests/pose_ref.py at every case of tests/pose_cases.py
(the cases tests/test_gpu_pose_forms.py runs on the kernel), the conditioning mask's 1 % cap, the sensitivity of the bars to eight
deliberately wrong variants of the reference, and the contract of the host's pose-slot order restated in Python."""
import numpy as np
import pytest

import pose_cases as PC
import pose_ref as R

oracle_case = PC.oracle_case


def family_worst(sge, name):
    rig, crowd, T, ticks = oracle_case(sge, name)
    worst = dict.fromkeys(R.FAMILIES, 0.0)
    for t in ticks:
        w, _ = R.local_ratios(t["local"], t["ref"])
        for f in worst:
            worst[f] = max(worst[f], w[f])
    return worst


@pytest.mark.parametrize("name", list(PC.RIGS))
def test_oracle_inside_every_bar(sge, name):
    """Clocks (discrete fields equal, float fields inside the counted bars, no comparison of a state machine met closer than 1e-5),
    the mask cap, locals inside the families' bars, models and palettes inside the derived bars."""
    rig, crowd, T, ticks = oracle_case(sge, name)
    bars = R.gpu_bars()
    for k, t in enumerate(ticks):
        tag = "%s tick %d" % (name, k)
        cw = R.check_clocks(t["after"], t["clocks"], tag)
        share = R.check_mask(t["ref"], tag)
        worst, ratio = R.local_ratios(t["local"], t["ref"])
        for f, v in worst.items():
            if v > bars[f]:
                e, b = np.unravel_index(int(np.argmax(np.where(t["ref"]["family"] == R.FAMILIES.index(f), ratio, 0))), ratio.shape)
                raise AssertionError(f"{tag}: family {f} at {v:.1f} of its unit, bar {bars[f]:.1f}; worst: row {crowd['names'][e]!r} bone {b}")
        model, mbar = R.model_f64(t["local"], rig.parent)
        mw = R.check_staged(t["model"], model, mbar, tag + " model")
        pal, pbar = R.palette_f64(t["model"], T.inv_bind.transpose(0, 2, 1).reshape(-1, 16))
        pw = R.check_staged(t["palette"], pal, pbar, tag + " palette")
        print(f"{tag}: clocks {cw:.2f} masked {share:.4f} locals " + " ".join(f"{f} {v:.1f}" for f, v in worst.items()) + f" | model {mw:.2f} palette {pw:.2f} of the derived bars")


def test_measured_oracle_figures_are_the_documented_ones(sge):
    """The basis of the GPU bars: the worst float32-oracle error per family over every case is what pose_ref.ORACLE_WORST says
    (rounded up to a tenth), the bars are 4 x that, and every one is below the 1e-5 (168 u on a unit entry) of the parity tests."""
    worst = dict.fromkeys(R.FAMILIES, 0.0)
    for name in PC.RIGS:
        for f, v in family_worst(sge, name).items():
            worst[f] = max(worst[f], v)
    print("worst float32-oracle error per family (u, u * mag):", {f: round(v, 2) for f, v in worst.items()})
    for f, v in worst.items():
        assert v <= R.ORACLE_WORST[f], (f, v)
        assert v >= 0.9 * R.ORACLE_WORST[f], (f, v, "the documented figure is stale")
        assert R.gpu_bars()[f] * R.U32 < 1e-5, f


def test_model_bar_at_depth_255_is_meaningful(sge):
    """The 256-bone chain: the product of absolute values P and the derived bar at the deepest bone, relative to the entry they bound."""
    rig, crowd, T, ticks = oracle_case(sge, "b256_chain")
    t = ticks[1]
    model, bar = R.model_f64(t["local"], rig.parent)
    scale = np.abs(model[:, 255, :3, :]).max((1, 2))
    rel = bar[:, 255, :3, :].max((1, 2)) / scale
    print(f"depth 255: bar / largest entry of the model matrix: max {rel.max():.3g} (= {rel.max() / R.U32:.0f} u)")
    assert rel.max() < 1e-3          # a wrong bone in the chain moves the model by far more (the parent mutation below)


# (variant, the rig whose crowd has a case where it matters)
MUTATIONS = [("swap_from_to", "b65_animated"), ("plain_root_slerp", "rotations"), ("harmonic_shift", "b64"), ("even_rule", "tail_even"),
             ("parent_minus_one", "b129"), ("action_unclamped", "b65_animated"), ("lean_side", "b65_static_leaf"), ("pre_side", "b64")]


@pytest.mark.parametrize("variant,name", MUTATIONS)
def test_a_wrong_reference_misses_the_bar_by_100x(sge, variant, name):
    """Sensitivity: from / to swapped, a plain slerp for the blending root, harmonic k taken as k - 1, `2 k <= count` for `2 k < count`,
    parent[i] - 1 for one bone, the action weight not clamped, the lean on the wrong side of the local, the pre-rotation on the wrong
    side. Each must be at least 100 bars away from the (correct) oracle somewhere.

    The plain slerp is the slerp without the shortest-arc choice, on the quaternions as the matrix conversion signs them: wrong where
    their dot is negative (the rotations rig's root between FallingIdle and Running, 210 degrees apart). The other half of the
    yaw-stable root is NOT something a bar can see, and no variant is made of it: left multiplication by a unit quaternion is an
    isometry of the 3-sphere, so yaw * slerp(yaw^-1 * from, yaw^-1 * to, w) equals slerp(from, to, w) up to rounding (the float32
    oracle is 0.19 of the bar from both, on the root that yaws from +179 to -179 degrees)."""
    rig, crowd, T, ticks = oracle_case(sge, name)
    bars = R.gpu_bars()
    far = 0.0
    for t in ticks:
        if variant == "parent_minus_one":
            model, bar = R.model_f64(t["local"], rig.parent, wrong_bone=rig.bone_count - 1)
            err = np.abs(R.mats(t["model"]) - model)
            far = max(far, float((err[bar > 0] / bar[bar > 0]).max()))
        else:
            ref = R.locals_f64(t["after"], T, mutate=(variant,))
            worst, _ = R.local_ratios(t["local"], ref)
            far = max(far, max(worst[f] / bars[f] for f in worst))
    print(f"{variant} on {name}: {far:.3g} bars away")
    assert far >= 100.0, (variant, far)


@pytest.mark.parametrize("name", [n for n in PC.RIGS if n.startswith("tail_")] + ["b1", "b2", "b128_chain"])
def test_reads_run_past_the_row(name):
    """From the rig's construction: the largest coefficient count uploaded (the table's row stride) is below the 2 KMAX + 1 floats
    the kernel reads of every row, so on these rigs every read leaves its row and the last row's reads end in the padded row."""
    rig = PC.RIGS[name][0]()
    assert PC.reads_leave_the_row(rig)
    if name.startswith("tail_"):
        want = {"c0": 0, "c1": 1, "c2": 2, "even": 10, "odd": 11, "full_row": 11, "absent": 255}[name[5:]]
        last = rig.profiles[-1]
        assert (last["coeffCount"][-1] == want).all() and max(p["order"] for p in rig.profiles) == 5
        assert last["order"] == (3 if name == "tail_full_row" else 5)


@pytest.mark.parametrize("name", list(PC.RIGS))
def test_pose_slot_contract(name):
    """rebuildPoseSlots is host code whose results (slot order, lastPassStatic, extraParentReady) no entry point reports: its
    contract restated in Python, on every rig, must give the form the rig is built for — asserted from the rig's construction.
    (A 65-bone chain has an admissible pick, its leaf, whose parent is finished a pass earlier: the ancestor-path walk of a later
    pass is reached by the 128- and 256-bone chains, where the last pass is full and the order is the index order.)
    The restatement itself is held to the contract's properties, stated independently of its loops: the slots are a permutation
    with bone 0 first; a reordered last pass never holds bone 0 or a bone together with its parent; a bone left out of it that is
    cheaper than one taken (static before animated, leaf before inner) touches a taken bone no dearer than itself; the order inside
    and outside the last pass is ascending; and the two flags follow from pass membership alone."""
    rig = PC.RIGS[name][0]()
    passes, static, ready, last = PC.RIGS[name][1]
    animated = np.zeros(rig.bone_count, bool)
    for p in rig.profiles:
        animated |= p["bonePresent"] != 0
    slots, got_static, got_ready = R.pose_slots(rig.parent, animated)
    B = rig.bone_count
    assert sorted(slots) == list(range(B)) and slots[0] == 0
    assert ((B + 63) // 64, got_static, got_ready) == (passes, static, ready)
    if last is not None:
        assert slots[64 * (passes - 1):] == last
    else:
        assert slots == list(range(B))
    # properties
    parent = [int(p) for p in rig.parent]
    pass_of = {b: s // 64 for s, b in enumerate(slots)}
    tail = slots[64 * (passes - 1):]
    head = slots[:64 * (passes - 1)]
    assert head == sorted(head) and tail == sorted(tail)
    if slots != list(range(B)):                                                   # a reordered last pass
        taken = set(tail)
        assert 0 not in taken and not any(parent[b] in taken for b in taken)
        kids = {b: [c for c in range(B) if parent[c] == b] for b in range(B)}
        cost = lambda b: (2 if animated[b] else 0) + (1 if kids[b] else 0)
        dearest = max(cost(b) for b in taken)
        for b in range(1, B):
            if b not in taken and cost(b) < dearest:
                near = [x for x in [parent[b]] + kids[b] if x in taken]
                assert near and min(cost(x) for x in near) <= cost(b), (b, near)
    assert got_ready == int(all(parent[b] < 0 or pass_of[parent[b]] < pass_of[b] for b in slots[64:]))
    assert got_static == int(passes > 1 and not any(animated[b] for b in tail))
