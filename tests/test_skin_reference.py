"""CPU companion of tests/test_gpu_skin_forms.py: the float64 reference and its bars (tests/skin_ref.py) against the oracle's
float32 skinning, at every (vertices, bones) shape the GPU tests use. Keeps the bars honest on a machine without a GPU."""
import numpy as np

import oracle_binding as ob
import test_gpu_skin_forms as forms
from skin_ref import check_streams, make_skin_case, rigid_shear_palette, skin_reference


def _shapes():
    shapes = {(V, forms.BONES) for _, V in forms.PLAIN_SHAPES} | {(513, forms.BONES), (1300, forms.BONES)}
    shapes |= {(257, 170), (257, 171), (257, 256)}
    shapes |= set(zip([1, 255, 256, 257, 5000, 33], [3, 65, 17, 256, 65, 1]))
    shapes |= {(V, forms.BONES) for _, V, _ in forms.FUSED_SHAPES}
    return sorted(shapes)


def test_skin_reference_bars_hold_for_the_oracle(sge):
    cpu = ob.oracle_engine()
    worst = [0.0, 0.0]
    try:
        for V, B in _shapes():
            case = make_skin_case(V, B, seed=1000 * B + V)
            assert int(case["boneIndices"].max()) == B - 1 or V < 12
            w = case["boneWeights"]
            if V >= 29:  # the rows fixed by vertex index are there
                assert ((w[:, 0] == 0) & (w[:, 1:] > 0).all(1)).any() and ((w[:, :3] == 0).all(1) & (w[:, 3] > 0)).any()
                assert (w[:, 3] < 0).any() and (case["boneIndices"] == case["boneIndices"][:, :1]).all(1).any()
            for translation in (0.5, 30.0):  # the pins test's palette, and one with the lever arm of a crowd in world space
                pal = rigid_shear_palette(B, np.random.default_rng(3 + V), translation)
                out = [np.zeros((V, 3), np.float32), np.zeros((V, 3), np.float32), np.zeros((V, 4), np.float32)]
                job = dict(sourcePositions=case["positions"].ctypes.data, sourceNormals=case["normals"].ctypes.data,
                           sourceTangents=case["tangents"].ctypes.data, sourceBoneIndices=case["boneIndices"].ctypes.data,
                           sourceBoneWeights=case["boneWeights"].ctypes.data, palette=pal.ctypes.data, paletteCount=B, vertexCount=V, dstBaseVertex=0)
                cpu.skinning_encode(out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, sge.abi.LAYOUT_PACKED, [job])
                rp, rd = check_streams(*out, skin_reference(case, pal), "oracle %d vertices %d bones" % (V, B))
                worst = [max(worst[0], rp), max(worst[1], rd)]
    finally:
        cpu.close()
    print("skin-forms oracle position %.3f direction %.3f" % tuple(worst))


def test_the_bars_catch_a_wrong_bone_and_a_dropped_influence():
    """What the bars are for: one vertex skinned with a neighbour's bone, or without its smallest influence, misses them."""
    V, B = 257, 33
    case = make_skin_case(V, B, seed=5)
    pal = rigid_shear_palette(B, np.random.default_rng(8), 30.0)
    ref = skin_reference(case, pal)
    good = [ref["pos"].astype(np.float32), ref["nrm"].astype(np.float32), ref["tan"].astype(np.float32)]
    check_streams(*good, ref, "the reference rounded to float32")
    v = int(np.flatnonzero((case["boneWeights"] > 0.05).sum(1) >= 2)[0])
    for what in ("bone", "influence"):
        bad = {k: np.array(a) for k, a in case.items()}
        j = int(np.argmax(bad["boneWeights"][v] > 0.05))
        if what == "bone":
            bad["boneIndices"][v, j] = (bad["boneIndices"][v, j] + 1) % B
        else:
            bad["boneWeights"][v, j] = 0.0
        wrong = skin_reference(bad, pal)
        try:
            check_streams(wrong["pos"].astype(np.float32), wrong["nrm"].astype(np.float32), wrong["tan"].astype(np.float32), ref, what)
        except AssertionError:
            continue
        raise AssertionError("a wrong %s at vertex %d passed the bars" % (what, v))
