"""TEST INFRASTRUCTURE: what the specular IBL tests share (test_ibl_reference.py on the CPU, test_gpu_render_ibl.py on the GPU):
the materials, the environment, the sampler's test directions and the frame's bar."""
import numpy as np

import ibl_ref as ir
import render_ibl_ref as rir
import render_scenes as rs
import render_tex_scenes as ts

ENV_SIZE, ENV_MIPS, LUT_SIZE = 16, 5, 16
SMALL = (48, 32)


def materials(sge):
    """render_scenes.materials with roughness over {0.05 (the mirror's clamp), 0.3, 0.7, 1} and metallic over {0, 0.5, 1}: 1 rough
    dielectric; 2 the mirror (the mirror path and the term coexist); 3 glass, half metallic; 4 the translucent sheets (the term
    composited in all three layers), fully rough; 5 the ground, fully rough, occlusion 0.8; 6 a rough metal."""
    m = rs.materials(sge)
    m["roughness"][3], m["metallic"][3] = 0.3, 0.5
    m["roughness"][4], m["metallic"][4] = 1.0, 0.5
    m["roughness"][5] = 1.0
    m["roughness"][6], m["metallic"][6] = 0.3, 1.0
    return m


def environment(sge):
    """The default cube at 16 with 5 levels and the default table at 16 x 16 -> (texels float16, levels, lut)."""
    texels = sge.ibl_default_env(ENV_SIZE, ENV_MIPS)
    return texels, ir.split_levels(texels, ENV_SIZE, ENV_MIPS), sge.ibl_default_brdf_lut(LUT_SIZE, 256)


def directions(seed=0, count=2000):
    """Directions for the cube sampler: random ones, the axes, all twelve edges and eight corners exactly (the ties) and within 1e-3
    of them, and hostile ones."""
    rng = np.random.default_rng(seed)
    out = [rng.normal(size=(count, 3)), rng.normal(size=(count // 4, 3)) * 1e-20, rng.normal(size=(count // 4, 3)) * 1e20]
    out.append(np.concatenate([np.eye(3), -np.eye(3)]))
    t = np.linspace(-1, 1, 9)
    edges = []
    for axis in range(3):  # the edge runs along `axis`; the other two components are +-1
        for s1 in (-1, 1):
            for s2 in (-1, 1):
                e = np.zeros((len(t), 3))
                e[:, axis], e[:, (axis + 1) % 3], e[:, (axis + 2) % 3] = t, s1, s2
                edges.append(e)
    edges = np.concatenate(edges)  # (t = +-1 are the eight corners)
    out += [edges, edges * 3.7, edges + rng.uniform(-1e-3, 1e-3, edges.shape), edges + rng.uniform(-1e-3, 1e-3, edges.shape)]
    odd = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -0.5])
    out.append(np.stack(np.meshgrid(odd, odd, odd), -1).reshape(-1, 3))
    return np.ascontiguousarray(np.concatenate(out), np.float32)


def lods(count, mip_count, seed=1):
    """0, the integers, mipCount - 1, halves between, below 0, above the top, non-finite, and random ones."""
    fixed = [0.0, -0.0, -1.0, -1e30, mip_count - 1, mip_count - 1 + 0.5, mip_count + 2, 1e30, np.nan, np.inf, -np.inf, 0.25]
    fixed += list(range(mip_count)) + [k + 0.5 for k in range(mip_count)]
    l = np.random.default_rng(seed).uniform(-0.5, mip_count - 0.5, count)
    k = np.arange(count)
    return np.where(k % 3 == 0, np.array(fixed)[(k // 3) % len(fixed)], l).astype(np.float32)


def random_cube(size, mip_count, seed):
    """Random halves: every finite bit pattern is allowed, among them denormals and the largest finite half."""
    n = 4 * sum(6 * s * s for s in ir.level_sizes(size, mip_count))
    bits = np.random.default_rng(seed).integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
    bits[(bits & 0x7C00) == 0x7C00] &= 0xBFFF  # (an exponent of all ones is inf / NaN: clear one exponent bit)
    bits[:8] = [0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x03FF, 0x0000, 0x8000, 0x3C00]
    return bits.view(np.float16).reshape(-1, 4)


# The worst |float32 restatement of the shading - float64| over stable pixels of the two static scenes with the term, measured on
# the CPU by test_ibl_reference.py between the float32 and the float64 shading of the reference (never from the GPU's image),
# rounded up to three digits.
RESTATEMENT_WORST = {
    "ibl": 1.48e-7,                    # measured 1.473e-7; no unstable pixel of 1,536 in the reference alone
    "ibl textured": 1.04e-7,           # 1.030e-7; none
    # the crowd with two mesh variants, measured beside the GPU by test_gpu_render_ibl.py (the reference needs the GPU's skinned
    # vertices), packed and padded16 alike; 40 of 1,536 pixels unstable in the reference alone
    "ibl variants": 4.88e-5,           # 4.878e-5
    "ibl textured variants": 2.16e-6,  # 2.155e-6
}


def colour_bar(name, base_bar, levels, spec_worst):
    """The existing scene's bar, plus 4 x the float32-against-float64 figure of the scene with the term, plus what R's coordinate bar
    may move the term by (render_ibl_ref.ibl_colour_term)."""
    return base_bar + 4 * RESTATEMENT_WORST[name] + rir.ibl_colour_term(levels, ENV_SIZE, spec_worst)
