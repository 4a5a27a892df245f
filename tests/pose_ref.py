"""TEST INFRASTRUCTURE: the float64 restatement of the pose stage and its error bars (tests/test_pose_reference.py on the CPU,
tests/test_gpu_pose_forms.py on the GPU). Plain numpy, float64 throughout, written from the Swift text
(Game/ProceduralPoseSystem.swift, Animation.swift:65-89, Skeleton.swift:189-217, Systems.swift:279-407 and :475-517); nothing here
calls the product, the oracle or their shared math header. u = 2**-24.

Stages, so that transcendental rounding and countable rounding are judged apart:

clocks_f64    LocomotionProfileSystem, ActionAnimationSystem and the clock / blend-weight head of PoseStackSystem on the state
              BEFORE a tick -> the state after it. Discrete fields (state, fromState, flags) must be equal. Float fields:
                  time, motionTime   6 u * max(|t| + |dt * rate|, cycle)   (product, sum, and on a transition quotient + product; the
                                     remainder itself is exact)
                  posePhase          that bar / cycle + 2 u                (the quotient, the clamp)
                  blendT, weight in  4 u * max(|value|, dt / duration)     (quotient, sum)
                  idleInertia, weight out  (12 + x) u * |value|, x = dt / halfLife   (the one extra allowance: pow(0.5, x) to 4 ulp = 8 u,
                                     its argument's rounding x ln 2 u, the quotient and the product)
              Every comparison the state machines make is reported with its relative margin; a case must keep 1e-5 away from each
              (or sit on it exactly, with exactly representable operands).
locals_f64    the local matrix of every bone from the DOWNLOADED post-tick state of the engine under test (a one-ulp clock difference
              then never cascades, and the reference takes the branch the code took): Fourier evaluation with the reference's
              loop-exit rule (term k is added iff k <= order and 2 k < count), pre-rotation, root fix, in-place, single-profile and
              no-motion branches with the bindLocal fallback, lerp / slerp under the smootherstep or idle-inertia weight, the
              yaw-stable root, the action layer, ground align on the pelvis, run lean.
model_f64, palette_f64   one stage each, redone in float64 from the float32 locals / models the engine stored.

Model bar (derived). model[i] = local[root] * ... * local[i], multiplied left to right, d = depth(i) products; the ancestor-path
walk and the one-product form with the parent's finished model (`extraParentReady`) are the same d products in the same order. An
entry of an affine product is 3 multiplies and 2 adds (rotation part) or 3 adds (translation: + c3 * 1 is exact), at most 4
roundings deep: |fl(A B) - A B| <= ((1 + u)**4 - 1) |A| |B|. Product k therefore adds at most 4 u |M_k-1| |L_k| <= 4 u P_k (1 + O(u))
with P_k = |L_0| |L_1| ... |L_k| the product of the absolute values, and what it adds is carried to the end by |L_k+1| ... |L_d|:
    |got - ref| <= 4 d u P_d (1 + O(d u)), stated as (4 d + 1) u P_d for d > 0 and 0 for the root (a copy)       per entry.
The bar is as meaningful as P_d: for rotations of large angle P grows like 1.4**d, so the chain rigs (depth 64 and 255) carry
rotations of a few degrees; test_pose_reference.py reports P and the bar at depth 255.

Palette bar (derived). palette = model * invBind: an entry is 4 multiplies and 3 adds, 4 roundings deep:
    |got - ref| <= 5 u (|M| |invBind|)                                                                               per entry.

Locals bar (measured, because of sincos up to 2 pi * 8, atan2, pow, sqrt and the quaternion round trip). Units: a rotation entry in
u (entries <= 1); a translation component c in u * mag[c], mag[c] = |rest[c]| + unitScale * (|rawRest[c]| + sum |coefficients| of
the terms the evaluation of axis c adds): the |delta| of the issue's unit taken as the sum of absolute values that bounds its
evaluation, since a delta that cancels to nothing (the root's, around a raw rest of several units) still carries the roundings of
its terms, and a unit that cancels with it would make the measured worst, and so the bar, arbitrarily large. Through a blend and
the action layer mag is carried per component (the larger of the two sides). Ground align and lean rotate the translation of their
bone: every component of the result sums all three components of the input, each times a rotation entry (<= 1) that carries its
own rounding, so there mag[c] becomes mag[0] + mag[1] + mag[2].
Per family, worst float32 ORACLE error over every case of tests/pose_cases.py (ORACLE_WORST below, asserted by
test_pose_reference.py), and the GPU bar = 4 x that: the device sincosf / atan2f / powf are specified to a few ulp where the host
libm delivers <= 1, and the kernel's no-blend shortcut drops one re-rounding.
    family        oracle worst   GPU bar    pose_kernel on the MI355X
    single        11.6           46.4       11.2
    blend          9.9           40.0       11.9
    yaw_root      10.5           42.4       10.5
    action        12.8           51.2        9.6
    pelvis_lean   14.5           58.0       11.3
All five bars are below the 168 u (1e-5) of the parity tests.

Conditioning mask: a (character, bone) entry is left out where the function itself is discontinuous or ill-conditioned:
    slerp with |dot(q0, q1)| < 0.02 (the shortest-arc sign switch)                        that bone
    the yaw atan2 of a vector shorter than 1e-3                                           the root
    |lengthSq(fh) - 0.0001| < 1e-5 (forward nearly vertical)                              pelvis and lean bone
    nProj shorter than 1e-3 before normalisation                                          pelvis and lean bone
    |runLeanWeight - 0.001| < 1e-5                                                        lean bone
    |action weight - 0.001| < 1e-6                                                        the character
At most 1 % of a case's entries may be masked and no whole bone or character (asserted per case on the CPU)."""
import numpy as np

U32 = 2.0 ** -24
PI32 = float(np.float32(float.fromhex("0x1.921fb4p+1")))    # Swift's Float.pi (rounded toward zero)
LOCO_IS_BLENDING, LOCO_PRESENT, MOTION_PRESENT, MOTION_LOOP, MOTION_IN_PLACE = 1, 2, 4, 8, 16
ACTION_PRESENT, ACTION_ACTIVE, ACTION_LOOP, ACTION_IN_PLACE, ACTION_EXITING, ACTION_HAS_DODGE = 1, 2, 4, 8, 16, 32
CTRL_GROUNDED_NEAR = 2
IDLE, WALK, RUN, FALLING = 0, 1, 2, 3
ABSENT = 255
FAMILIES = ("single", "blend", "yaw_root", "action", "pelvis_lean")
F_SINGLE, F_BLEND, F_YAW, F_ACTION, F_PELVIS = range(5)

# worst float32-oracle error per family in the units above, over every case, rounded up to a tenth (measured and asserted by
# test_pose_reference.py: 11.60 single, 9.94 blend, 10.52 yaw_root, 12.75 action, 14.45 pelvis_lean) -> GPU bars 46.4, 40.0, 42.4, 51.2,
# 58.0 u (2.8e-6, 2.4e-6, 2.5e-6, 3.1e-6, 3.5e-6 on a unit entry; the parity tests' 1e-5 is 168 u)
ORACLE_WORST = {"single": 11.6, "blend": 10.0, "yaw_root": 10.6, "action": 12.8, "pelvis_lean": 14.5}
GPU_FACTOR = 4.0


def gpu_bars():
    return {k: GPU_FACTOR * v for k, v in ORACLE_WORST.items()}


# ---- small float64 algebra -------------------------------------------------------------------------------------------------

def mats(a):
    """[..][16] column-major float4x4 -> [..][4][4] float64, row-major (M[r][c])."""
    a = np.asarray(a, np.float64)
    return np.swapaxes(a.reshape(a.shape[:-1] + (4, 4)), -1, -2)


def _axis_rot(rad, axis):
    c, s = np.cos(rad), np.sin(rad)
    R = np.zeros(np.shape(rad) + (3, 3))
    i, j, k = axis, (axis + 1) % 3, (axis + 2) % 3
    R[..., i, i] = 1.0
    R[..., j, j] = c; R[..., j, k] = -s
    R[..., k, j] = s; R[..., k, k] = c
    return R


def rotation_xyz_degrees(deg):
    """Skeleton.swift:212-217: Rz * (Ry * Rx), radians_from_degrees = deg / 180 * Float.pi."""
    rad = np.asarray(deg, np.float64) / 180.0 * PI32
    return _axis_rot(rad[..., 2], 2) @ (_axis_rot(rad[..., 1], 1) @ _axis_rot(rad[..., 0], 0))


def quat_from_rot(R):
    """Unit quaternion (x, y, z, w) of rotation matrices [..][3][3], by the largest of the four squared components (the sign is
    whatever that branch gives: slerp takes the shortest arc, and entries where the sign decides are masked)."""
    R = np.asarray(R, np.float64)
    m = lambda r, c: R[..., r, c]
    tr = m(0, 0) + m(1, 1) + m(2, 2)
    four = np.stack([1 + m(0, 0) - m(1, 1) - m(2, 2), 1 - m(0, 0) + m(1, 1) - m(2, 2), 1 - m(0, 0) - m(1, 1) + m(2, 2), 1 + tr], -1)
    pick = np.argmax(four, -1)
    big = 0.5 * np.sqrt(np.take_along_axis(four, pick[..., None], -1)[..., 0])
    f = 0.25 / big
    cand = np.stack([
        np.stack([big, (m(0, 1) + m(1, 0)) * f, (m(0, 2) + m(2, 0)) * f, (m(2, 1) - m(1, 2)) * f], -1),
        np.stack([(m(0, 1) + m(1, 0)) * f, big, (m(1, 2) + m(2, 1)) * f, (m(0, 2) - m(2, 0)) * f], -1),
        np.stack([(m(0, 2) + m(2, 0)) * f, (m(1, 2) + m(2, 1)) * f, big, (m(1, 0) - m(0, 1)) * f], -1),
        np.stack([(m(2, 1) - m(1, 2)) * f, (m(0, 2) - m(2, 0)) * f, (m(1, 0) - m(0, 1)) * f, big], -1)], -2)
    q = np.take_along_axis(cand, pick[..., None, None], -2)[..., 0, :]
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def rot_from_quat(q):
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def quat_mul(p, q):
    px, py, pz, pw = (p[..., k] for k in range(4))
    qx, qy, qz, qw = (q[..., k] for k in range(4))
    return np.stack([pw * qx + px * qw + py * qz - pz * qy, pw * qy - px * qz + py * qw + pz * qx,
                     pw * qz + px * qy - py * qx + pz * qw, pw * qw - px * qx - py * qy - pz * qz], -1)


def quat_conj(q):
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def quat_angle_axis(angle, axis):
    h = 0.5 * angle
    return np.concatenate([np.sin(h) * np.asarray(axis, np.float64), [np.cos(h)]])


def quat_from_rot_signed(R):
    """The quaternion of ONE rotation matrix with the sign the reference's conversion gives it (the published rule of
    simd_quaternion(matrix): w >= 0 when the trace is >= 0, else the component of the largest diagonal entry positive). Only the
    plain-slerp variant of the sensitivity test needs the sign; everything else is sign-free."""
    q = quat_from_rot(R)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    lead = 3 if tr >= 0 else int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
    return -q if q[lead] < 0 else q


def slerp(q0, q1, t, shortest=True):
    """simd_slerp: the shortest arc (q1 negated when dot < 0); shortest=False: the plain slerp, along whichever arc the signs of the
    two quaternions span. -> (q, |dot|)."""
    d = np.sum(q0 * q1, -1, keepdims=True)
    if shortest:
        q1 = np.where(d < 0, -q1, q1)
    ang = 2.0 * np.arctan2(np.linalg.norm(q0 - q1, axis=-1, keepdims=True), np.linalg.norm(q0 + q1, axis=-1, keepdims=True))
    small = ang < 1e-9
    sa = np.where(small, 1.0, np.sin(ang))
    k0 = np.where(small, 1.0 - t, np.sin((1.0 - t) * ang) / sa)
    k1 = np.where(small, t, np.sin(t * ang) / sa)
    q = k0 * q0 + k1 * q1
    return q / np.linalg.norm(q, axis=-1, keepdims=True), np.abs(d[..., 0])


def _compose(R, t):
    M = np.zeros(R.shape[:-2] + (4, 4))
    M[..., :3, :3] = R
    M[..., :3, 3] = t
    M[..., 3, 3] = 1.0
    return M


def cycle_of(profile):
    return max(float(np.float32(profile["cycleDuration"])), float(np.float32(0.001)))


# ---- rebuildPoseSlots, restated ----------------------------------------------------------------------------------------------

def pose_slots(parent, animated):
    """The contract of the host's slot order: the bones of a partly filled last pass are the cheapest the rig has (static leaves,
    static inner bones, animated leaves, the rest; the highest index first; never bone 0, never a bone with its parent or child), or
    index order when no such pick exists. -> (slots, lastPassStatic, extraParentReady)."""
    B = len(parent)
    passes, extra = (B + 63) // 64, B - 64 * ((B + 63) // 64 - 1)
    is_extra = np.zeros(B, bool)
    if passes > 1 and extra < 64:
        has_child = np.zeros(B, bool)
        for i in range(B):
            if parent[i] >= 0:
                has_child[parent[i]] = True
        picked = 0
        for cls in range(4):
            for i in range(B - 1, 0, -1):
                if picked >= extra:
                    break
                if (2 if animated[i] else 0) + (1 if has_child[i] else 0) != cls or is_extra[i]:
                    continue
                if parent[i] >= 0 and is_extra[parent[i]]:
                    continue
                if any(is_extra[j] and parent[j] == i for j in range(i + 1, B)):
                    continue
                is_extra[i] = True
                picked += 1
        if picked != extra:
            is_extra[:] = False
    slots = [i for i in range(B) if not is_extra[i]] + [i for i in range(B) if is_extra[i]]
    slot_of = {b: s for s, b in enumerate(slots)}
    ready = all(parent[slots[s]] < 0 or slot_of[parent[slots[s]]] // 64 < s // 64 for s in range(64, B))
    static = passes > 1 and not any(animated[slots[s]] for s in range(64 * (passes - 1), B))
    return slots, int(static), int(ready)


# ---- clocks -------------------------------------------------------------------------------------------------------------------

def _grounded_next(cur, speed, L):
    g = IDLE if cur == FALLING else cur
    if g == IDLE:
        return RUN if speed >= L["runEnterSpeed"] else (WALK if speed >= L["idleExitSpeed"] else IDLE)
    if g == WALK:
        return RUN if speed >= L["runEnterSpeed"] else (IDLE if speed < L["idleEnterSpeed"] else WALK)
    if g == RUN:
        if speed < L["runExitSpeed"]:
            return IDLE if speed < L["idleEnterSpeed"] else WALK
        return RUN
    return FALLING


def clocks_f64(before, dt, profiles):
    """before: dict(bodies, controllers, locomotion, actions) of structured arrays -> list (one per character) of
    dict(loco={field: value}, act={...}, lbar={field: bar}, abar={...}, margins=[(what, relative margin)])."""
    dt = float(np.float32(dt))
    cyc_of = [cycle_of(p) for p in profiles]
    out = []
    for e in range(len(before["locomotion"])):
        L = {k: (np.array(before["locomotion"][k][e], np.float64) if before["locomotion"].dtype[k].kind == "f" else before["locomotion"][k][e].copy())
             for k in before["locomotion"].dtype.names}
        A = {k: (float(before["actions"][k][e]) if before["actions"].dtype[k].kind == "f" else int(before["actions"][k][e])) for k in before["actions"].dtype.names}
        body, C = before["bodies"][e], before["controllers"][e]
        flags, state, from_state = int(L["flags"]), int(L["state"]), int(L["fromState"])
        time = [float(x) for x in L["time"]]
        tbar = [0.0] * 4
        margins = []
        near = lambda what, a, b: margins.append((what, abs(a - b) / max(abs(b), 1e-30)))
        has_loco, has_motion = bool(flags & LOCO_PRESENT), bool(flags & MOTION_PRESENT)
        cyc = [cyc_of[int(p)] for p in L["profile"]]
        motion_time, blend_t, inertia = float(L["motionTime"]), float(L["blendT"]), float(L["idleInertia"])
        if has_loco and has_motion:                                              # Systems.swift:326-406
            speed = float(np.hypot(body["linearVelocity"][0], body["linearVelocity"][2]))
            for k in ("idleEnterSpeed", "idleExitSpeed", "runEnterSpeed", "runExitSpeed"):
                near("speed vs " + k, speed, float(L[k]))
            Lf = {k: float(L[k]) for k in ("idleEnterSpeed", "idleExitSpeed", "runEnterSpeed", "runExitSpeed")}
            airborne = not (int(C["flags"]) & CTRL_GROUNDED_NEAR)
            if airborne:
                near("groundDistance vs fallMinDropHeight", float(C["groundDistance"]), float(L["fallMinDropHeight"]))
                high = float(C["groundDistance"]) >= float(L["fallMinDropHeight"])
                nxt = FALLING if (state == FALLING or high) else _grounded_next(state, speed, Lf)
            else:
                nxt = _grounded_next(state, speed, Lf)
            if nxt != state:
                from_phase = max(0.0, min(time[state] / cyc[state], 1.0))
                time[nxt] = from_phase * cyc[nxt]
                tbar[nxt] = 3 * U32 * cyc[nxt]
                from_state, state = state, nxt
                flags |= LOCO_IS_BLENDING
                blend_t = 0.0
                if nxt == IDLE:
                    inertia = 1.0
            motion_time = time[state]
        mbar = tbar[state] if (has_loco and has_motion) else 0.0
        # ActionAnimationSystem, Systems.swift:475-517
        aflags, atime, aw = A["flags"], A["time"], A["weight"]
        abar = {"time": 0.0, "weight": 0.0}
        if dt > 0 and (aflags & ACTION_PRESENT) and (aflags & ACTION_ACTIVE):
            cycle = cyc_of[A["profile"]]
            cap = cycle
            if aflags & ACTION_HAS_DODGE:
                cap = max(min(A["dodgeEnd"], cycle), float(np.float32(0.001)))
            exiting = bool(aflags & ACTION_EXITING)
            if not exiting:
                step = dt * A["playbackRate"]
                t2 = atime + step
                abar["time"] = 6 * U32 * max(abs(atime) + abs(step), cap)
                if aflags & ACTION_LOOP:
                    near("action time vs wrap", t2, round(t2 / cap) * cap if round(t2 / cap) else cap)
                    atime = float(np.fmod(t2, cap))
                else:
                    near("action time vs cap", t2, cap)
                    atime = t2
                    if t2 >= cap:
                        atime, exiting = cap, True
                        abar["time"] = 0.0
            active = True
            if exiting:
                x = dt / max(A["blendOutHalfLife"], float(np.float32(0.001)))
                aw = aw * 0.5 ** x
                abar["weight"] = (12 + x) * U32 * abs(aw)
                near("action weight vs 0.001", aw, float(np.float32(0.001)))
                if aw <= float(np.float32(0.001)):
                    aw, active, exiting = 0.0, False, False
                    abar["weight"] = 0.0
            else:
                inc = dt / max(A["blendInTime"], float(np.float32(0.001)))
                near("action weight vs 1", aw + inc, 1.0)
                aw = min(aw + inc, 1.0)
                abar["weight"] = 0.0 if aw == 1.0 else 4 * U32 * max(abs(aw), inc)
            aflags &= ~(ACTION_ACTIVE | ACTION_EXITING)
            aflags |= (ACTION_ACTIVE if active else 0) | (ACTION_EXITING if exiting else 0)
        # the clock head of PoseStackSystem, ProceduralPoseSystem.swift:36-90 / 224-234
        loop = bool(flags & MOTION_LOOP)
        rate = float(L["playbackRate"])
        lbar = {"blendT": 0.0, "idleInertia": 0.0}
        pose_phase = float(L["posePhase"])
        pbar = 0.0

        def advance(t, cycle, bar0, what):
            t2 = t + dt * rate
            bar = bar0 + 6 * U32 * max(abs(t) + abs(dt * rate), cycle)
            if loop:
                m = round(t2 / cycle)
                near(what + " vs wrap", t2, m * cycle if m else cycle)
                return float(np.fmod(t2, cycle)), bar
            near(what + " vs cycle", t2, cycle)
            return (cycle, 0.0) if t2 >= cycle else (t2, bar)

        if has_loco and has_motion:
            for s in range(4):
                time[s], tbar[s] = advance(time[s], cyc[s], tbar[s], "time[%d]" % s)
            if flags & LOCO_IS_BLENDING:
                blending = True
                if state == IDLE:
                    x = dt / max(float(L["idleInertiaHalfLife"]), float(np.float32(0.001)))
                    inertia = inertia * 0.5 ** x
                    lbar["idleInertia"] = (12 + x) * U32 * abs(inertia)
                    near("idleInertia vs 0.001", inertia, float(np.float32(0.001)))
                    if inertia <= float(np.float32(0.001)):
                        inertia, blend_t, blending = 0.0, 1.0, False
                        lbar["idleInertia"] = 0.0
                else:
                    inc = dt / max(float(L["blendTime"]), float(np.float32(0.001)))
                    near("blendT vs 1", blend_t + inc, 1.0)
                    blend_t = min(blend_t + inc, 1.0)
                    lbar["blendT"] = 0.0 if blend_t == 1.0 else 4 * U32 * max(abs(blend_t), inc)
                    if blend_t >= 1.0:
                        blending = False
                if not blending:
                    flags &= ~LOCO_IS_BLENDING
            pose_phase = max(0.0, min(time[state] / cyc[state], 1.0))
            pbar = tbar[state] / cyc[state] + 2 * U32
        elif has_motion:
            cycle = cyc_of[int(L["motionProfile"])]
            motion_time, mbar = advance(motion_time, cycle, 0.0, "motionTime")
            pose_phase = max(0.0, min(motion_time / cycle, 1.0))
            pbar = mbar / cycle + 2 * U32
        out.append({"loco": {"time": time, "state": state, "fromState": from_state, "flags": flags, "motionTime": motion_time,
                             "blendT": blend_t, "idleInertia": inertia, "posePhase": pose_phase},
                    "lbar": dict(lbar, time=tbar, motionTime=mbar, posePhase=pbar),
                    "act": {"time": atime, "weight": aw, "flags": aflags}, "abar": abar, "margins": margins})
    return out


def check_clocks(got, ref, name, min_margin=1e-5):
    """Downloaded post-tick state against clocks_f64's. -> worst error / bar over the float fields."""
    worst = 0.0
    for e, r in enumerate(ref):
        for what, m in r["margins"]:
            assert m == 0.0 or m >= min_margin, (name, e, what, m, "the case sits on a state-machine comparison")
        for key, fields, bars in (("locomotion", r["loco"], r["lbar"]), ("actions", r["act"], r["abar"])):
            for f, want in fields.items():
                have = got[key][f][e]
                if f in ("state", "fromState", "flags"):
                    assert int(have) == int(want), (name, "character", e, key, f, int(have), int(want))
                    continue
                err = np.abs(np.asarray(have, np.float64) - np.asarray(want, np.float64))
                bar = np.asarray(bars[f], np.float64)
                assert np.all(err <= bar), (name, "character", e, key, f, have, want, err.tolist(), bar.tolist())
                if np.any(bar > 0):
                    worst = max(worst, float(np.max(err[bar > 0] / bar[bar > 0])) if np.ndim(err) else float(err / bar))
    return worst


# ---- locals -------------------------------------------------------------------------------------------------------------------

class RigTables:
    """The float32 inputs of the pose stage as float64 arrays: what the skeleton build produced and the profile tables."""

    def __init__(self, rig, built):
        self.B = rig.bone_count
        self.parent = np.asarray(rig.parent, np.int64)
        self.rest = np.asarray(built["restTranslation"], np.float64).reshape(self.B, 3)
        self.raw = np.asarray(rig.translations, np.float32).astype(np.float64).reshape(self.B, 3)
        self.pre = rotation_xyz_degrees(np.asarray(rig.pre_rotation_degrees, np.float32).astype(np.float64))
        self.root_fix = mats(np.asarray(built["rootRotationFix"]).reshape(16))[:3, :3]
        self.bind = mats(np.asarray(built["bindLocal"]).reshape(self.B, 16))
        self.inv_bind = mats(np.asarray(built["invBindModel"]).reshape(self.B, 16))
        self.unit = float(np.float32(rig.unit_scale))
        self.pelvis, self.lean = int(rig.pelvis_index), int(rig.lean_index)
        self.profiles = [{"order": int(p["order"]), "cycle": cycle_of(p), "present": np.asarray(p["bonePresent"]) != 0,
                          "count": np.asarray(p["coeffCount"], np.int64), "coeffs": np.asarray(p["coeffs"], np.float32).astype(np.float64)}
                         for p in rig.profiles]
        self.depth = np.zeros(self.B, np.int64)
        for i in range(self.B):
            self.depth[i] = 0 if self.parent[i] < 0 else self.depth[self.parent[i]] + 1


def eval_profile(T, k, phase, in_place, mutate=()):
    """One profile at one phase -> (t [B][3], R [B][3][3], present [B], mag [B][3]); a bone the profile has no entry for evaluates to the
    defaults (rest translation, pre-rotation alone), which is what the blending branch uses for it (:153-192)."""
    P = T.profiles[k]
    p = max(0.0, min(float(phase), 1.0))
    ks = np.arange(1, 9)
    ang = 2 * PI32 * (ks - 1 if "harmonic_shift" in mutate else ks) * p                       # Animation.swift:73
    cs, sn = np.cos(ang), np.sin(ang)
    cnt, co = P["count"], P["coeffs"]
    has = (cnt != ABSENT) & P["present"][:, None]
    limit = (2 * ks[None, None, :] <= cnt[..., None]) if "even_rule" in mutate else (2 * ks[None, None, :] < cnt[..., None])
    inc = (ks[None, None, :] <= P["order"]) & limit & (cnt[..., None] != ABSENT)
    a, b = co[..., 1:17:2], co[..., 2:17:2]
    val = np.where(cnt > 0, co[..., 0], 0.0) + np.sum(np.where(inc, a * cs + b * sn, 0.0), -1)
    absval = np.where(cnt > 0, np.abs(co[..., 0]), 0.0) + np.sum(np.where(inc, np.abs(a) + np.abs(b), 0.0), -1)
    raw = np.where(has[:, :3], val[:, :3], T.raw)
    deg = np.where(has[:, 3:], val[:, 3:], 0.0)
    t = T.rest + (raw - T.raw) * T.unit
    mag = np.abs(T.rest) + np.where(has[:, :3], T.unit * (np.abs(T.raw) + absval[:, :3]), 0.0)
    if in_place:
        t[0, 0], t[0, 2] = T.rest[0, 0], T.rest[0, 2]
    anim = rotation_xyz_degrees(deg)
    R = anim @ T.pre if "pre_side" in mutate else T.pre @ anim
    R[0] = T.root_fix @ R[0]
    return t, R, P["present"].copy(), mag


def _single(T, k, phase, in_place, mutate):
    t, R, present, mag = eval_profile(T, k, phase, in_place, mutate)
    loc = _compose(R, t)
    loc[~present] = T.bind[~present]
    return loc, np.where(present[:, None], mag, np.abs(T.bind[:, :3, 3]))


def chain(local, parent, wrong_bone=None):
    """Skeleton.buildModelTransforms (:189-203) on [B][4][4]."""
    model = np.empty_like(local)
    for i in range(len(parent)):
        p = parent[i] - 1 if i == wrong_bone else parent[i]
        model[i] = local[i] if p < 0 else model[p] @ local[i]
    return model


def locals_f64(state, T, mutate=()):
    """state: dict(bodies, controllers, locomotion, actions) AFTER the tick. -> dict(local [n][B][4][4], family [n][B], mask [n][B],
    mag [n][B][3]); `mutate`: names of the deliberately wrong variants test_pose_reference.py applies."""
    n, B = len(state["locomotion"]), T.B
    local = np.zeros((n, B, 4, 4))
    family = np.zeros((n, B), np.int64)
    mask = np.zeros((n, B), bool)
    mag = np.zeros((n, B, 3))
    for e in range(n):
        L, A, body, C = state["locomotion"][e], state["actions"][e], state["bodies"][e], state["controllers"][e]
        flags = int(L["flags"])
        has_loco, has_motion = bool(flags & LOCO_PRESENT), bool(flags & MOTION_PRESENT)
        in_place = bool(flags & MOTION_IN_PLACE)
        run_lean = 0.0
        if has_loco and has_motion:                                              # :36-223
            blending = bool(flags & LOCO_IS_BLENDING)
            st = int(L["state"])
            cyc = [T.profiles[int(p)]["cycle"] for p in L["profile"]]
            phase = [max(0.0, min(float(L["time"][s]) / cyc[s], 1.0)) for s in range(4)]
            frm, to = (int(L["fromState"]) if blending else st), st
            w = 1.0
            if blending:
                if st == IDLE:
                    w = 1.0 - max(0.0, min(float(L["idleInertia"]), 1.0))
                else:
                    t = max(0.0, min(float(L["blendT"]), 1.0))
                    w = t * t * t * (t * (t * 6 - 15) + 10)
            if blending:
                run_lean = w if st == RUN else ((1.0 - w) if int(L["fromState"]) == RUN else 0.0)
            else:
                run_lean = 1.0 if st == RUN else 0.0
            if "swap_from_to" in mutate:
                frm, to = to, frm
            ft, fR, _, fm = eval_profile(T, int(L["profile"][frm]), phase[frm], in_place, mutate)
            tt, tR, _, tm = eval_profile(T, int(L["profile"][to]), phase[to], in_place, mutate)
            t = ft + (tt - ft) * w
            fq, tq = quat_from_rot(fR), quat_from_rot(tR)
            q, dots = slerp(fq, tq, w)
            family[e] = F_BLEND if blending else F_SINGLE
            if blending:
                mask[e] |= dots < 0.02
                if "plain_root_slerp" in mutate:
                    q[0], _ = slerp(quat_from_rot_signed(fR[0]), quat_from_rot_signed(tR[0]), w, shortest=False)
                else:                                                            # the yaw-stable root, :206-215
                    zx, zz = fR[0][0, 2], fR[0][2, 2]
                    yaw_q = quat_angle_axis(np.arctan2(zx, zz), (0, 1, 0))
                    pr, _ = slerp(quat_mul(quat_conj(yaw_q), fq[0]), quat_mul(quat_conj(yaw_q), tq[0]), w)
                    q[0] = quat_mul(yaw_q, pr)
                    mask[e, 0] |= np.hypot(zx, zz) < 1e-3
                family[e, 0] = F_YAW
            local[e] = _compose(rot_from_quat(q), t)
            mag[e] = np.maximum(fm, tm)
        elif has_motion:                                                         # :224-276
            k = int(L["motionProfile"])
            phase = max(0.0, min(float(L["motionTime"]) / T.profiles[k]["cycle"], 1.0))
            local[e], mag[e] = _single(T, k, phase, in_place, mutate)
        else:                                                                    # :277-284
            local[e], mag[e] = T.bind, np.abs(T.bind[:, :3, 3])
        aflags, aw = int(A["flags"]), float(A["weight"])
        if (aflags & ACTION_PRESENT) and (aflags & ACTION_ACTIVE):
            if abs(aw - float(np.float32(0.001))) < 1e-6:
                mask[e] = True
        if (aflags & ACTION_PRESENT) and (aflags & ACTION_ACTIVE) and aw > float(np.float32(0.001)):    # :286-338
            k = int(A["profile"])
            phase = max(0.0, min(float(A["time"]) / T.profiles[k]["cycle"], 1.0))
            act, amag = _single(T, k, phase, bool(aflags & ACTION_IN_PLACE), mutate)
            w = aw if "action_unclamped" in mutate else max(0.0, min(aw, 1.0))
            run_lean *= 1 - w
            t = local[e][:, :3, 3] + (act[:, :3, 3] - local[e][:, :3, 3]) * w
            q, dots = slerp(quat_from_rot(local[e][:, :3, :3]), quat_from_rot(act[:, :3, :3]), w)
            mask[e] |= dots < 0.02
            local[e] = _compose(rot_from_quat(q), t)
            mag[e] = np.maximum(mag[e], amag)
            family[e] = F_ACTION
        if T.pelvis >= 0:                                                        # :344-394
            tq = np.asarray(body["transformRotation"], np.float64)
            fwd = _act(tq, np.array([0.0, 0.0, -1.0]))
            fh = np.array([fwd[0], 0.0, fwd[2]])
            lsq = float(fh @ fh)
            ill = abs(lsq - float(np.float32(0.0001))) < 1e-5
            fh = fh / np.sqrt(lsq) if lsq > float(np.float32(0.0001)) else np.array([0.0, 0.0, -1.0])
            align = np.eye(3)
            if int(C["flags"]) & CTRL_GROUNDED_NEAR:
                up = np.array([0.0, 1.0, 0.0])
                right = np.cross(up, fh); right /= np.linalg.norm(right)
                g = np.asarray(C["groundNormal"], np.float64)
                n_proj = g - right * (g @ right)
                ill = ill or np.linalg.norm(n_proj) < 1e-3
                n_proj = n_proj / np.linalg.norm(n_proj)
                angle = np.arctan2(np.cross(up, n_proj) @ right, up @ n_proj) * float(np.float32(0.33))
                align = rot_from_quat(quat_angle_axis(angle, right))
            A4 = _compose(align, np.zeros(3))
            local[e, T.pelvis] = A4 @ local[e, T.pelvis]
            family[e, T.pelvis] = F_PELVIS
            mag[e, T.pelvis] = mag[e, T.pelvis].sum()
            mask[e, T.pelvis] |= ill
            if run_lean > float(np.float32(0.001)) and T.lean >= 0:
                model = chain(local[e], T.parent)
                rw = model[T.lean][:3, 0] / np.linalg.norm(model[T.lean][:3, 0])
                pi = T.parent[T.lean]
                rl = rot_from_quat(quat_conj(quat_from_rot(model[pi][:3, :3]))) @ rw if pi >= 0 else rw
                lean = _compose(rot_from_quat(quat_angle_axis(10.0 / 180.0 * PI32 * run_lean, rl)), np.zeros(3))
                local[e, T.lean] = local[e, T.lean] @ lean if "lean_side" in mutate else lean @ local[e, T.lean]
                family[e, T.lean] = F_PELVIS
                if T.lean != T.pelvis:
                    mag[e, T.lean] = mag[e, T.lean].sum()
                mask[e, T.lean] |= ill
            if T.lean >= 0 and abs(run_lean - float(np.float32(0.001))) < 1e-5:
                mask[e, T.lean] = True
    return {"local": local, "family": family, "mask": mask, "mag": mag}


def _act(q, v):
    """simd_act: t = 2 cross(imag, v); v + real t + cross(imag, t)."""
    t = 2.0 * np.cross(q[:3], v)
    return v + q[3] * t + np.cross(q[:3], t)


def local_ratios(got_local, ref):
    """Engine locals [n][B][16] float32 against locals_f64's -> dict family -> worst error in the family's units (masked entries
    left out), and the [n][B] array of the ratios."""
    G = mats(got_local)
    err = np.abs(G - ref["local"])
    rot = err[..., :3, :3].max((-1, -2)) / U32
    tr = np.where(err[..., :3, 3] == 0, 0.0, err[..., :3, 3] / (U32 * np.maximum(ref["mag"], 1e-300))).max(-1)
    assert (G[..., 3, :] == np.array([0.0, 0.0, 0.0, 1.0])).all(), "the bottom row of a local matrix is (0, 0, 0, 1)"
    ratio = np.where(ref["mask"], 0.0, np.maximum(rot, tr))
    return {name: float(ratio[ref["family"] == k].max()) if (ref["family"] == k).any() else 0.0 for k, name in enumerate(FAMILIES)}, ratio


def check_mask(ref, name):
    m = ref["mask"]
    assert m.mean() <= 0.01, (name, "masked share", float(m.mean()))
    assert not m.all(0).any(), (name, "a whole bone is masked", np.flatnonzero(m.all(0)).tolist())
    assert not m.all(1).any(), (name, "a whole character is masked", np.flatnonzero(m.all(1)).tolist())
    return float(m.mean())


# ---- model and palette: one stage each, from the engine's own float32 matrices, with derived bars -------------------------------

def model_f64(locals32, parent, wrong_bone=None):
    """locals32 [n][B][16] -> (model [n][B][4][4], bar [n][B][4][4]); the bar of the module docstring."""
    Lm = mats(locals32)
    n, B = Lm.shape[:2]
    model, P = np.empty_like(Lm), np.empty_like(Lm)
    depth = np.zeros(B, np.int64)
    for i in range(B):
        p = parent[i] - 1 if i == wrong_bone else parent[i]
        if p < 0:
            model[:, i], P[:, i] = Lm[:, i], np.abs(Lm[:, i])
        else:
            depth[i] = depth[p] + 1
            model[:, i], P[:, i] = model[:, p] @ Lm[:, i], P[:, p] @ np.abs(Lm[:, i])
    bar = np.where(depth > 0, 4 * depth + 1, 0)[None, :, None, None] * U32 * P
    return model, bar


def palette_f64(model32, inv_bind32):
    """model32 [n][B][16], inv_bind32 [B][16] -> (palette [n][B][4][4], bar)."""
    M, I = mats(model32), mats(inv_bind32)
    return M @ I[None], 5 * U32 * (np.abs(M) @ np.abs(I)[None])


def check_staged(got, want, bar, name):
    """-> worst error / bar (0 where the bar is 0 and the entry is equal)."""
    G = mats(got)
    err = np.abs(G - want)
    bad = err > bar
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, err / np.maximum(bar, 1e-300), 0))), err.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} entries beyond the derived bar; worst at (character, bone, row, col) {i}: "
                             f"got {G[i]!r} ref {want[i]!r} |d| {err[i]:.3g} bar {bar[i]:.3g}")
    pos = bar > 0
    return float((err[pos] / bar[pos]).max()) if pos.any() else 0.0
