"""TEST INFRASTRUCTURE: the rigs, profiles and single-character rows that put one case on every form of the pose kernel, shared by
tests/test_pose_reference.py (the float32 oracle on the CPU) and tests/test_gpu_pose_forms.py (the kernel). Pose stages only: bodies,
controllers, locomotion and action states are uploaded directly, nothing is simulated. Every crowd is ticked with dt = 0, 1/64, 1/64
(1/64 and the cycle durations are exactly representable, so "lands exactly on the cycle" and "reaches 1 on this tick" mean it)."""
import numpy as np

import pose_ref as R
from scenes import ExplicitRig

DT = 1.0 / 64.0
CYCLES = (0.5, 0.75, 1.0, 0.625, 0.875)          # idle, walk, run, fall, action: dyadic
STAGES = 8 | 16 | 32                              # STAGE_LOCOMOTION | STAGE_ACTION | STAGE_POSE


def _tree(bones):
    return np.array([-1] + [(i - 1) // 3 for i in range(1, bones)], np.int32)


def _chain(bones):
    return np.arange(-1, bones - 1, dtype=np.int32)


def _profile(rng, bones, order, cycle, absent=(), translate=(0,), amp=25.0, ragged=True, full=None):
    """Random Fourier rows: rotation on every present bone, translation on `translate`; a tenth of the axes nil, a fifth ragged."""
    present = np.ones(bones, np.uint8)
    present[list(absent)] = 0
    present[0] = 1
    count = np.full((bones, 6), 255, np.uint8)
    coeffs = np.zeros((bones, 6, 17), np.float32)
    ncoef = 1 + 2 * order if full is None else full
    for b in range(bones):
        if not present[b]:
            continue
        for a in [3, 4, 5] + ([0, 1, 2] if b in translate else []):
            u = rng.uniform()
            if ragged and u < 0.1:
                continue
            c = int(rng.integers(0, ncoef + 1)) if (ragged and u < 0.3) else ncoef
            count[b, a] = c
            coeffs[b, a, :c] = rng.normal(0, amp if a >= 3 else 3.0, c) / (1 + np.arange(c))
    return {"order": order, "cycleDuration": cycle, "bonePresent": present, "coeffCount": count, "coeffs": coeffs}


def _rig(bones, parent, orders, seed, absent_all=(), small=None, pelvis=0, lean=-1, translate=(0,), profiles=5, cycles=CYCLES):
    rng = np.random.default_rng(seed)
    tr = rng.uniform(-8, 8, (bones, 3))
    # small: pre-rotations of +-small degrees and amplitudes of 1.5 small degrees (the chains, whose product of |matrices| must stay bounded)
    pre = rng.uniform(-1, 1, (bones, 3)) * small if small else rng.uniform(-40, 40, (bones, 3))
    profs = []
    for k in range(profiles):
        # bone 3 has no entry in Idle: absent in the from-profile of the idle -> walk rows, in the to-profile of the -> idle rows
        absent = list(absent_all) + ([3] if (k == 0 and bones > 4) else [])
        profs.append(_profile(rng, bones, orders[k % len(orders)], cycles[k % len(cycles)], absent,
                              translate, amp=1.5 * small if small else 25.0))
    return ExplicitRig(parent, tr, pre, profs, pelvis_index=pelvis, lean_index=lean)


def _rig16():
    """16 profiles (the most a context takes) on 63 bones: non-root translation in profile 15 only (bit 15 of the kernel's mask);
    profile 13 has cycleDuration 0 and profile 14 0.0005 (both clamp to 0.001); no pelvis bone."""
    rng = np.random.default_rng(1663)
    bones = 63
    profs = [_profile(rng, bones, 4, CYCLES[k % 5], [3] if k == 0 else [], translate=(0, 10, 62) if k == 15 else (0,)) for k in range(16)]
    profs[13]["cycleDuration"], profs[14]["cycleDuration"] = 0.0, 0.0005
    profs[15]["coeffCount"][62, :3] = 9
    profs[15]["coeffs"][62, :3, :9] = rng.normal(0, 3.0, (3, 9))
    return ExplicitRig(_tree(bones), rng.uniform(-8, 8, (bones, 3)), rng.uniform(-40, 40, (bones, 3)), profs, pelvis_index=-1, lean_index=1)


def _tail_rig(kind):
    """Three bones, every profile of order 5 (so the launch is pose_kernel<8>, which reads 17 floats of every row) and no row longer
    than 11 coefficients (so the table's row stride is 11 and EVERY read runs six floats into the next row): the last axis rows of the
    LAST bone of the LAST profile, whose reads run into the one padded row at the end of the table, have the coefficient count named
    by `kind` (`full_row`: the last profile is of order 3 and its rows hold the full 11)."""
    rng = np.random.default_rng(77)
    order = 5
    cnt = {"c0": 0, "c1": 1, "c2": 2, "even": 2 * order, "odd": 2 * order + 1, "full_row": 2 * order + 1, "absent": 255}[kind]
    profs = [_profile(rng, 3, order, CYCLES[k], ragged=False, translate=(0, 2)) for k in range(5)]
    if kind == "full_row":
        profs[4]["order"] = 3
    for p in profs:
        p["coeffCount"][2, :] = cnt
        p["coeffs"][2] = 0
        if cnt != 255:
            p["coeffs"][2, :, :cnt] = rng.normal(0, 20.0, (6, cnt)) / (1 + np.arange(cnt))
    return ExplicitRig(_tree(3), rng.uniform(-8, 8, (3, 3)), rng.uniform(-40, 40, (3, 3)), profs, pelvis_index=0, lean_index=1)


def reads_leave_the_row(rig):
    """True when the kernel's reads of 2 KMAX + 1 floats per row run past the rows of this rig's table (KMAX = 4 for orders <= 4,
    else 8; the row stride is the largest coefficient count uploaded)."""
    kmax = 4 if max(p["order"] for p in rig.profiles) <= 4 else 8
    stride = max(int(p["coeffCount"][p["coeffCount"] != 255].max(initial=1)) for p in rig.profiles)
    return stride < 2 * kmax + 1


def _const(deg_xyz):
    row = np.zeros((6, 17), np.float32)
    row[3:, 0] = deg_xyz
    return row


def _rot_rig():
    """Chosen rotations, no pre-rotation and no root fix: constant coefficients (count 1). Idle = the from-profile, Walking = the
    to-profile of the rows that blend. Bones: 1-3 about 175 degrees about x / y / z (the three trace < 0 branches of the matrix ->
    quaternion conversion); 4, 5 trace = +1e-3 / -1e-3; 6 from == to; 7 from / to 1e-3 rad apart; 8, 9 dot(from, to) = +0.05 / -0.05
    (about x: 2 acos(+-0.05)); the root yaws +179 degrees in Idle and -179 in Walking. FallingIdle and Running turn the root 100 and
    -110 degrees about x (plus a little y): 210 degrees apart, both of trace >= 0, so their quaternions have a negative dot and
    the shortest arc between them is NOT the one a slerp without the sign choice takes."""
    bones = 12
    t_plus = np.degrees(np.arccos((1e-3 - 1) / 2))
    t_minus = np.degrees(np.arccos((-1e-3 - 1) / 2))
    idle = {1: (175, 0, 0), 2: (0, 175, 0), 3: (0, 0, 175), 4: (t_plus, 0, 0), 5: (0, t_minus, 0), 6: (33, -20, 70), 7: (10, 20, 30),
            8: (0, 0, 0), 9: (0, 0, 0), 0: (4, 179, -3), 10: (20, 30, 40), 11: (-50, 10, 5)}
    walk = dict(idle)
    walk.update({1: (174, 3, 0), 2: (2, 176, 0), 3: (0, 3, 174), 7: (10 + np.degrees(1e-3), 20, 30),
                 8: (np.degrees(2 * np.arccos(0.05)), 0, 0), 9: (np.degrees(2 * np.arccos(-0.05)), 0, 0), 0: (-5, -179, 2)})
    profs = []
    rng = np.random.default_rng(5)
    for k in range(5):
        src = idle if k in (0, 3) else walk
        count = np.full((bones, 6), 255, np.uint8)
        count[:, 3:] = 1
        coeffs = np.stack([_const(src[b]) for b in range(bones)])
        if k in (2, 4):
            coeffs[:, 3:, 0] += rng.uniform(-30, 30, (bones, 3)).astype(np.float32)
        if k in (2, 3):
            coeffs[0, 3:, 0] = (-110, 25, 0) if k == 2 else (100, 20, 0)
        profs.append({"order": 4, "cycleDuration": CYCLES[k], "bonePresent": np.ones(bones, np.uint8), "coeffCount": count, "coeffs": coeffs})
    return ExplicitRig(_tree(bones), rng.uniform(-8, 8, (bones, 3)), np.zeros((bones, 3)), profs, pelvis_index=-1, lean_index=-1,
                       root_fix_degrees=(0, 0, 0))


# name -> (builder, what rebuildPoseSlots must make of it: passes, lastPassStatic, extraParentReady, bones of the last pass or None)
RIGS = {
    "b1": (lambda: _rig(1, _tree(1), (1,), 11, pelvis=0, lean=0), (1, 0, 1, None)),
    "b2": (lambda: _rig(2, _tree(2), (5,), 12, pelvis=0, lean=0), (1, 0, 1, None)),
    "b63_16profiles": (_rig16, (1, 0, 1, None)),
    "b33_pelvis1": (lambda: _rig(33, _tree(33), (4,), 13, pelvis=1, lean=4), (1, 0, 1, None)),       # a pelvis with a parent, the lean below it
    "b64": (lambda: _rig(64, _tree(64), (8,), 14, pelvis=0, lean=-1, translate=(0, 5, 63)), (1, 0, 1, None)),
    "b65_static_leaf": (lambda: _rig(65, _tree(65), (4,), 15, absent_all=(64,), lean=1), (2, 1, 1, [64])),
    "b65_animated": (lambda: _rig(65, _tree(65), (8, 2), 16, lean=1), (2, 0, 1, [64])),
    "b65_chain": (lambda: _rig(65, _chain(65), (4,), 17, small=1.0, lean=40), (2, 0, 1, [64])),
    "b128_chain": (lambda: _rig(128, _chain(128), (5,), 18, small=1.0, lean=40), (2, 0, 0, None)),
    "b129": (lambda: _rig(129, _tree(129), (4,), 19, lean=1, translate=(0, 7, 128)), (3, 0, 1, [128])),
    "b193_static_leaf": (lambda: _rig(193, _tree(193), (8,), 20, absent_all=(192,), lean=1), (4, 1, 1, [192])),
    "b256_chain": (lambda: _rig(256, _chain(256), (4,), 21, small=0.05, lean=40), (4, 0, 0, None)),
    "b256_tree": (lambda: _rig(256, _tree(256), (8,), 22, lean=1), (4, 0, 1, None)),
    "rotations": (_rot_rig, (1, 0, 1, None)),
}
for _kind in ("c0", "c1", "c2", "even", "odd", "full_row", "absent"):
    RIGS["tail_" + _kind] = ((lambda k=_kind: _tail_rig(k)), (1, 0, 1, None))

FLAGS_LOCO = R.LOCO_PRESENT | R.MOTION_PRESENT | R.MOTION_LOOP | R.MOTION_IN_PLACE


def _yaw_quat(yaw, pitch=0.0):
    """Rotation about y by yaw, then (in the rotated frame) about x by pitch, as (x, y, z, w)."""
    qy = np.array([0, np.sin(yaw / 2), 0, np.cos(yaw / 2)])
    qx = np.array([np.sin(pitch / 2), 0, 0, np.cos(pitch / 2)])
    return R.quat_mul(qy, qx)


def rows(pkg, rig, seed=3):
    """The crowd of single-character rows (the same on every rig) -> dict(bodies, controllers, locomotion, actions, names)."""
    abi, assets = pkg.abi, pkg.assets
    P = len(rig.profiles)
    cyc = [R.cycle_of(p) for p in rig.profiles]
    prof = (0, 1 % P, 2 % P, 3 % P)
    act_prof = 4 % P
    specs = []

    def row(name, **kw):
        specs.append(dict(kw, name=name))

    decay = 0.5 ** (DT / 0.18)
    run = dict(state=R.RUN, speed=8.0)
    row("time 0, idle")
    row("lands exactly on the cycle, loop", state=R.WALK, speed=4.0, time_exact=True)
    row("lands exactly on the cycle, no loop", state=R.WALK, speed=4.0, time_exact=True, loop=False)
    row("clamped at phase 1, no loop", state=R.WALK, speed=4.0, time_full=True, loop=False)
    row("blend starts this tick (walk -> run)", state=R.WALK, speed=8.0)
    row("blend starts this tick (idle -> walk)", state=R.IDLE, speed=4.0)
    row("idle -> walk, mid blend", state=R.WALK, speed=4.0, from_state=R.IDLE, blend_t=0.6)
    row("blend reaches 1 on this tick", state=R.RUN, speed=8.0, from_state=R.WALK, blend_t=0.9375, blend_time=0.25)
    row("idle inertia lands on 0.0011", state=R.IDLE, speed=0.0, from_state=R.WALK, inertia=0.0011 / decay)
    row("idle inertia lands on 0.0009", state=R.IDLE, speed=0.0, from_state=R.WALK, inertia=0.0009 / decay)
    row("falling entered by drop height", grounded=False, ground_distance=60.0, **run)
    row("falling left", state=R.FALLING, speed=0.0)
    row("from == to while blending", state=R.WALK, speed=4.0, from_state=R.WALK, blend_t=0.3)
    row("run -> walk", state=R.RUN, speed=3.0)
    row("walk -> run, mid blend", from_state=R.WALK, blend_t=0.5, **run)
    row("falling -> run, mid blend", from_state=R.FALLING, blend_t=0.45, **run)
    row("run -> idle, mid blend", state=R.IDLE, speed=0.0, from_state=R.RUN, inertia=0.6)
    row("action weight 0.0011", action=dict(weight=0.0011), **run)
    row("action weight 0.0009", action=dict(weight=0.0009), **run)
    row("action weight 1 cancels the lean", action=dict(weight=1.0), **run)
    row("dodge cap shorter than the cycle", action=dict(weight=0.7, dodge=0.25, time=0.25 - DT), state=R.WALK, speed=4.0)
    row("looping action", action=dict(weight=0.5, loop=True, time=cyc[act_prof] - 1.5 * DT), state=R.WALK, speed=4.0)
    row("action exits and dies on this tick", action=dict(weight=0.00105, exiting=True), state=R.WALK, speed=4.0)
    row("action in place, motion not", action=dict(weight=0.6, in_place=True), in_place=False, state=R.WALK, speed=4.0)
    row("motion in place, action not", action=dict(weight=0.6, in_place=False), state=R.WALK, speed=4.0)
    row("action weight above 1, exiting", action=dict(weight=1.5, exiting=True), **run)
    row("action over a blend", action=dict(weight=0.35), from_state=R.WALK, blend_t=0.4, **run)
    row("not grounded", grounded=False, ground_distance=1.0, **run)
    row("normal exactly up", **run)
    row("normal 40 degrees across forward", normal=("across", 40.0), **run)
    row("normal 40 degrees along forward", normal=("along", 40.0), yaw=0.7, **run)
    row("forward nearly vertical, fallback taken", pitch=np.radians(89.6), normal=("along", 20.0), **run)
    row("forward nearly vertical, fallback not taken", pitch=np.radians(89.2), normal=("along", 20.0), **run)
    row("motion profile alone", loco=False, time0=0.2)
    row("motion profile alone, no loop, clamped", loco=False, loop=False, time_full=True)
    row("no motion: bind pose", loco=False, motion=False)
    row("locomotion profile 15", profiles=(P - 1, 1 % P, 2 % P, 3 % P), time0=0.11)
    row("action profile 15", action=dict(weight=0.45, profile=P - 1), state=R.WALK, speed=4.0)
    if P == 16:
        row("cycleDuration 0", loco=False, motion_profile=13, time0=0.0)
        row("cycleDuration 0.0005", loco=False, motion_profile=14, time0=0.0002)
        row("cycleDuration 0 as an action", action=dict(weight=0.5, profile=13), state=R.WALK, speed=4.0)
    n = len(specs)
    rng = np.random.default_rng(seed)
    bodies = assets.default_bodies(n, np.zeros((n, 3)))
    ctrl = assets.default_controller_state(n)
    loco = np.zeros(n, abi.locomotion_dtype)
    act = np.zeros(n, abi.action_dtype)
    loco["idleEnterSpeed"], loco["idleExitSpeed"], loco["runEnterSpeed"], loco["runExitSpeed"] = 0.15, 0.3, 6.0, 5.0
    loco["fallMinDropHeight"], loco["blendTime"], loco["blendT"] = 50.0, 0.2, 1.0
    loco["idleInertiaHalfLife"], loco["playbackRate"] = 0.18, 1.0
    act["playbackRate"], act["blendInTime"], act["blendOutHalfLife"] = 1.0, 0.08, 0.18
    for e, s in enumerate(specs):
        state = s.get("state", R.IDLE)
        L = loco[e:e + 1]
        L["profile"] = s.get("profiles", prof)
        c4 = [cyc[int(p)] for p in L["profile"][0]]
        # times: a quarter-odd multiple of 1/256 inside the cycle, so no wrap or clamp is met by accident
        L["time"] = [np.floor(rng.uniform(0.1, 0.8) * c * 64) / 64 + 1.0 / 256 for c in c4]
        if "time0" in s:
            L["time"][0, state] = s["time0"]
        if s.get("time_exact"):
            L["time"][0, state] = c4[state] - DT
        if s.get("time_full"):
            L["time"][0, state] = c4[state]
        if s["name"].startswith("time 0"):
            L["time"] = 0.0
        L["state"], L["fromState"] = state, s.get("from_state", state)
        fl = 0
        if s.get("loco", True):
            fl |= R.LOCO_PRESENT
        if s.get("motion", True):
            fl |= R.MOTION_PRESENT
        if s.get("loop", True):
            fl |= R.MOTION_LOOP
        if s.get("in_place", True):
            fl |= R.MOTION_IN_PLACE
        if "blend_t" in s or "inertia" in s:
            fl |= R.LOCO_IS_BLENDING
            L["blendT"] = s.get("blend_t", 0.0)
            L["idleInertia"] = s.get("inertia", 0.0)
        L["blendTime"] = s.get("blend_time", 0.2)
        L["flags"] = fl
        L["motionProfile"] = s.get("motion_profile", int(L["profile"][0, state]))
        L["motionTime"] = L["time"][0, state]
        yaw = s.get("yaw", rng.uniform(-3, 3))
        q = _yaw_quat(yaw, s.get("pitch", 0.0))
        bodies["transformRotation"][e] = q
        bodies["rotation"][e] = q
        sp = s.get("speed", 0.0)
        bodies["linearVelocity"][e] = (sp * np.cos(yaw), -1.0, sp * np.sin(yaw))
        if s.get("grounded", True):
            ctrl["flags"][e] = abi.CTRL_GROUNDED | abi.CTRL_GROUNDED_NEAR
        ctrl["groundDistance"][e] = s.get("ground_distance", 0.0)
        if "normal" in s:
            how, degs = s["normal"]
            fwd = R.rot_from_quat(_yaw_quat(yaw)) @ np.array([0, 0, -1.0])
            side = np.cross([0, 1.0, 0], fwd)
            d = fwd if how == "along" else side
            ctrl["groundNormal"][e] = np.cos(np.radians(degs)) * np.array([0, 1.0, 0]) + np.sin(np.radians(degs)) * d
        a = s.get("action")
        A = act[e:e + 1]
        A["profile"] = act_prof
        A["flags"] = R.ACTION_PRESENT
        if a:
            A["profile"] = a.get("profile", act_prof)
            A["weight"] = a["weight"]
            A["time"] = a.get("time", 0.1)
            A["flags"] = (R.ACTION_PRESENT | R.ACTION_ACTIVE | (R.ACTION_LOOP if a.get("loop") else 0) | (R.ACTION_EXITING if a.get("exiting") else 0)
                          | (R.ACTION_IN_PLACE if a.get("in_place", True) else 0) | (R.ACTION_HAS_DODGE if "dodge" in a else 0))
            A["dodgeEnd"] = a.get("dodge", 0.0)
    return {"bodies": bodies, "controllers": ctrl, "locomotion": loco, "actions": act, "names": [s["name"] for s in specs]}


def tiny_mesh():
    """Three vertices on bone 0 (the pose stages read no mesh; a context is set up with one all the same)."""
    return {"positions": np.eye(3, dtype=np.float32), "normals": np.eye(3, dtype=np.float32),
            "tangents": np.array([[0, 1, 0, 1], [0, 0, 1, 1], [1, 0, 0, -1]], np.float32),
            "boneIndices": np.zeros((3, 4), np.uint16), "boneWeights": np.tile(np.array([1, 0, 0, 0], np.float32), (3, 1))}


def run_case(pkg, eng, rig, crowd, ticks=(0.0, DT, DT), sub=None):
    """Uploads the rig and the crowd into a fresh engine and ticks the pose stages. Yields, per tick, dict(dt, before, after, palette,
    model, local) with the downloaded states around the tick. sub = (first, count): the ticks after the first run on that range only."""
    eng.set_option(pkg.abi.OPT_STORE_POSE_DEBUG, 1)
    built = eng.upload_skeleton(rig)
    eng.upload_profiles(rig.profiles)
    eng.upload_skinned_mesh(tiny_mesh())
    n = len(crowd["locomotion"])
    eng.resize(n)
    eng.upload(bodies=crowd["bodies"], params=pkg.assets.default_controller_params(n), controllers=crowd["controllers"],
               intents=pkg.assets.default_intents(n), locomotion=crowd["locomotion"], actions=crowd["actions"])
    for k, dt in enumerate(ticks):
        eng.synchronize()
        before = eng.download(what=("bodies", "controllers", "locomotion", "actions"))
        first, count = sub if (sub and k > 0) else (0, n)
        eng.tick(dt=dt, stages=STAGES, first=first, count=count if sub and k > 0 else 0)
        eng.synchronize()
        after = eng.download(what=("bodies", "controllers", "locomotion", "actions"))
        pal, mod, loc = eng.palettes(model=True, local=True)
        yield {"dt": dt, "before": before, "after": after, "palette": pal, "model": mod, "local": loc, "built": built, "range": (first, count)}


_ORACLE = {}


def oracle_case(pkg, name):
    """The float32 oracle's three ticks of one rig's crowd with the float64 references of each tick (once per session)
    -> (rig, crowd, RigTables, ticks)."""
    if name not in _ORACLE:
        from oracle_binding import oracle_engine
        rig = RIGS[name][0]()
        crowd = rows(pkg, rig)
        eng = oracle_engine()
        try:
            ticks = list(run_case(pkg, eng, rig, crowd))
        finally:
            eng.close()
        T = R.RigTables(rig, ticks[0]["built"])
        for t in ticks:
            t["clocks"] = R.clocks_f64(t["before"], t["dt"], rig.profiles)
            t["ref"] = R.locals_f64(t["after"], T)
        _ORACLE[name] = (rig, crowd, T, ticks)
    return _ORACLE[name]
