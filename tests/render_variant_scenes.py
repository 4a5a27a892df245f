"""TEST INFRASTRUCTURE: the scene of the shaded frame over a crowd with genuinely different mesh variants
(tests/test_gpu_variant_scene.py): where the 37 characters of the variant world stand, their materials, the statics, the lights and
the camera, and the scene's float32 restatement figure, kept like those of tests/render_scenes.py.

The characters of the synthetic world are some 400 units across. Rows of four stand 420 apart, every other row shifted by half a
step, so that behind a character of one variant stands one of another; rows 2.. stand behind the mirror wall, out of sight. Row 0:
characters 0 and 1 are translucent (a character of another variant shows through), 3 is glass (the refraction path leaves through
another variant), 2 (the one-triangle variant) is rough. A mirror wall behind row 1 reflects the characters; a translucent sheet stands in front of characters
0 and 1; two lights, the first with its shadow walk through the translucent occluders."""
import numpy as np

import render_scenes as rs

CHARS = 37
STEP = 420.0


def instances():
    """[CHARS][4][4] row-major model matrices."""
    m = np.tile(np.eye(4, dtype=np.float32), (CHARS, 1, 1))
    c = np.arange(CHARS)
    row = c // 4
    m[:, 0, 3] = (c % 4) * STEP + (row % 2) * STEP / 2
    m[:, 2, 3] = -row * STEP - np.where(row >= 2, 3000.0, 0.0)
    return m


def crowd_materials():
    out = np.full(CHARS, 6, np.int32)
    out[0], out[1], out[3] = 4, 4, 3
    return out


def statics():
    """-> meshes, mesh_of, matrices [S][4][4], material_of: ground, mirror wall, translucent sheet."""
    meshes = {0: rs.quad(1.0), 1: rs.box()}
    mesh_of = [0, 1, 1]
    mats = [rs.transform((6000, 1, 6000), 0.0, (600, -330, -500)), rs.transform((3600, 1400, 30), 0.0, (700, 200, -900)),
            rs.transform((700, 600, 6), 0.1, (200, 0, 380))]
    return meshes, mesh_of, np.array(mats, np.float32), [5, 2, 4]


def lights(sge):
    l = np.zeros(2, sge.abi.render_light_dtype)
    l["direction"] = [(-0.35, -1.0, -0.45), (0.5, -0.6, -0.4)]
    l["intensity"] = [2.2, 0.6]
    l["color"] = [(1.0, 0.95, 0.85), (0.6, 0.7, 1.0)]
    l["enabled"] = [1, 1]
    l["maxDistance"] = [1e5, 0.0]
    return l


def camera():
    return np.array([760.0, 420.0, 1700.0]), np.array([700.0, -20.0, -200.0])


SIZE = (48, 32)  # (at 24 x 16 the reference alone leaves 3.6 % of the pixels unstable, above the 3 % the rule allows; here 2.99 %)

# The worst |float32 restatement of the shading - float64| over stable pixels (render_ref: path A shaded in float32 against path A
# shaded in float64), measured on the CPU over the GPU's skinned vertices of this scene and rounded up to three digits. The colour
# bar is 4 x the figure.
RESTATEMENT_WORST = {"variant crowd packed": 3.60e-7}  # measured 3.593e-7; 46 of 1,536 pixels unstable in the reference alone


def colour_bar(name):
    return 4 * RESTATEMENT_WORST[name]
