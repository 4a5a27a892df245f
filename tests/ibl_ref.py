"""TEST INFRASTRUCTURE: specular IBL (include/sge_amd_render_ibl.h) written from the Metal and Swift text: eval_spec_ibl
(RayTracing.metalinc:88-104) with the cube sampler (mip-linear, bilinear, seamless across edges) and the table sampler in numpy
float32 in the order the header pins and in float64; and IBLResources.init (Game/IBLResources.swift) in float64.

`variant` selects a deliberately wrong restatement (test_ibl_reference.py shows that each misses its bar):
  the table:   "k_direct" (k = (a + 1)^2 / 8), "swap_ab" (A and B swapped), "unclamped_ndotv" (no max(., 0.001) on nDotV);
  the cube:    "flip_v" (the faces' v sign flipped in cubeDirection);
  the sampler: "face_clamp" (taps clamped per face instead of the seamless taps), "round_level" (level = round(mip)),
               "reflect_v" (R = reflect(V, N))."""
import numpy as np

from render_ref import _dot, _sat

FACES = 6


def level_sizes(size, mip_count):
    return [max(size >> m, 1) for m in range(mip_count)]


def split_levels(texels, size, mip_count):
    """float16 [texels][4] as sge_render_env_upload takes it -> a list of [6][n][n][4] float16, one per level."""
    t = np.asarray(texels).reshape(-1, 4)
    out, at = [], 0
    for n in level_sizes(size, mip_count):
        out.append(t[at:at + 6 * n * n].reshape(6, n, n, 4))
        at += 6 * n * n
    assert at == len(t)
    return out


def join_levels(levels):
    return np.concatenate([np.asarray(l).reshape(-1, 4) for l in levels])


def cube_direction(face, u, v, flip_v=False):
    """IBLResources.swift:93-104, not normalised. face [k] int; u, v [k]."""
    if flip_v:
        v = -v
    one = np.ones_like(u)
    table = [(one, -v, -u), (-one, -v, u), (u, one, v), (u, -one, -v), (u, -v, one), (-u, -v, -one)]
    out = np.zeros(u.shape + (3,), u.dtype)
    for f, comps in enumerate(table):
        sel = face == f
        for k in range(3):
            out[..., k] = np.where(sel, comps[k], out[..., k])
    return out


def cube_coord(d):
    """The header's face selection and the inverse of cubeDirection -> (face, u, v) in d's type."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    with np.errstate(all="ignore"):
        fx = (ax >= ay) & (ax >= az)
        fy = ~fx & (ay >= az)
        face = np.where(fx, np.where(x < 0, 1, 0), np.where(fy, np.where(y < 0, 3, 2), np.where(z < 0, 5, 4)))
        us = [-z / ax, z / ax, x / ay, x / ay, x / az, -x / az]
        vs = [-y / ax, -y / ax, z / ay, -z / ay, -y / az, -y / az]
    u, v = np.zeros_like(x), np.zeros_like(x)
    for f in range(6):
        u = np.where(face == f, us[f], u)
        v = np.where(face == f, vs[f], v)
    return face, u, v


def _level_sample(level, face, u, v, ft, variant):
    """level [6][n][n][>=3] in ft; one bilinear sample with the seamless taps."""
    n = level.shape[1]
    fn = ft(n)

    def coord(c):
        x = np.fmin(np.fmax(((c + ft(1)) * ft(0.5)) * fn - ft(0.5), ft(-0.5)), fn - ft(0.5))
        x0 = np.floor(x)
        return x0.astype(np.int64), (x - x0).astype(ft)

    def tap(i, j):
        if variant == "face_clamp":
            return level[face, np.clip(j, 0, n - 1), np.clip(i, 0, n - 1), :3]
        outside = (i < 0) | (i >= n) | (j < 0) | (j >= n)
        uc = (ft(2) * (i.astype(ft) + ft(0.5))) / fn - ft(1)
        vc = (ft(2) * (j.astype(ft) + ft(0.5))) / fn - ft(1)
        f2, u2, v2 = cube_coord(cube_direction(face, uc, vc))
        with np.errstate(all="ignore"):
            i2 = np.clip(np.nan_to_num(np.floor(((u2 + ft(1)) * ft(0.5)) * fn)).astype(np.int64), 0, n - 1)
            j2 = np.clip(np.nan_to_num(np.floor(((v2 + ft(1)) * ft(0.5)) * fn)).astype(np.int64), 0, n - 1)
        f, ii, jj = np.where(outside, f2, face), np.where(outside, i2, np.clip(i, 0, n - 1)), np.where(outside, j2, np.clip(j, 0, n - 1))
        return level[f, jj, ii, :3]

    with np.errstate(all="ignore"):
        x0, fx = coord(u)
        y0, fy = coord(v)
    fx, fy = fx[:, None], fy[:, None]
    one = ft(1)
    t00, t10, t01, t11 = tap(x0, y0), tap(x0 + 1, y0), tap(x0, y0 + 1), tap(x0 + 1, y0 + 1)
    with np.errstate(all="ignore"):
        top = t00 * (one - fx) + t10 * fx
        bot = t01 * (one - fx) + t11 * fx
        return top * (one - fy) + bot * fy


def env_sample(levels, dirs, lods, ft=np.float32, variant=None):
    """envMap.sample(samp, d, level(lod)).xyz: levels from split_levels; dirs [k][3]; lods [k] -> ft [k][3]."""
    lv = [np.asarray(l).astype(ft) for l in levels]
    mc = len(lv)
    d = np.asarray(dirs, ft).reshape(-1, 3)
    lod = np.asarray(lods, ft).reshape(-1)
    with np.errstate(all="ignore"):
        mip = np.fmin(np.fmax(lod, ft(0)), ft(mc - 1))
        if variant == "round_level":
            l0 = np.rint(mip).astype(np.int64)
            l1, fl = l0, np.zeros_like(mip)
        else:
            l0 = np.floor(mip).astype(np.int64)
            l1 = np.minimum(l0 + 1, mc - 1)
            fl = (mip - l0.astype(ft)).astype(ft)
    face, u, v = cube_coord(d)
    c0, c1 = np.zeros((len(d), 3), ft), np.zeros((len(d), 3), ft)
    for l in range(mc):
        for which, out in ((l0, c0), (l1, c1)):
            sel = which == l
            if sel.any():
                out[sel] = _level_sample(lv[l], face[sel], u[sel], v[sel], ft, variant)
    with np.errstate(all="ignore"):
        return c0 * (ft(1) - fl)[:, None] + c1 * fl[:, None]


def lut_sample(lut, uvs, ft=np.float32):
    """brdfLUT.sample(samp, uv).xy: the coordinates and filter of render_tex_ref.sample over float texels. lut [H][W][>=2]."""
    t = np.asarray(lut).astype(ft)[..., :2]
    H, W = t.shape[:2]
    uv = np.asarray(uvs, ft).reshape(-1, 2)

    def axis(c, size):
        x = np.fmin(np.fmax(c * ft(size) - ft(0.5), ft(0)), ft(size - 1))
        i0 = np.floor(x).astype(np.int64)
        return i0, np.minimum(i0 + 1, size - 1), (x - i0.astype(ft)).astype(ft)

    with np.errstate(all="ignore"):
        x0, x1, fx = axis(uv[:, 0], W)
        y0, y1, fy = axis(uv[:, 1], H)
        fx, fy = fx[:, None], fy[:, None]
        one = ft(1)
        top = t[y0, x0] * (one - fx) + t[y0, x1] * fx
        bot = t[y1, x0] * (one - fx) + t[y1, x1] * fx
        return top * (one - fy) + bot * fy


def reflect_dir(N, V, variant=None):
    """R = reflect(-V, N) with the reflect of sge_amd_render.h."""
    I = V if variant == "reflect_v" else -V
    two = N.dtype.type(2)
    return I - N * (two * _dot(N, I))[..., None]


def eval_spec_ibl(levels, lut, N, V, roughness, metallic, base, ft=np.float32, variant=None):
    """:88-104 -> ft [k][3] (before the occlusion factor of :380)."""
    N, V, base = np.asarray(N, ft), np.asarray(V, ft), np.asarray(base, ft)
    rough, metal = np.asarray(roughness, ft), np.asarray(metallic, ft)
    nov = _sat(_dot(N, V))
    Rd = reflect_dir(N, V, variant)
    mip = rough * np.maximum(ft(len(levels) - 1), ft(0))
    pre = env_sample(levels, Rd, mip, ft, variant)
    brdf = lut_sample(lut, np.stack([nov, rough], -1), ft)
    F0 = ft(0.04) + (base - ft(0.04)) * metal[:, None]
    return pre * (F0 * brdf[:, :1] + brdf[:, 1:2])


def tie_margin(d):
    """How far a direction is from a tie of the face selection, as a fraction of its largest component: the gap between the two
    largest absolute components."""
    a = np.sort(np.abs(np.asarray(d, np.float64)), axis=-1)
    return (a[..., 2] - a[..., 1]) / np.maximum(a[..., 2], 1e-300)


def adjacent_step(levels):
    """The largest difference between two texels that one bilinear footprint joins, over the levels given: every 2 x 2 footprint of
    every face, x0 and y0 from -1 to n - 1, its taps outside the face resolved to the texels the seamless rule reads."""
    worst = 0.0
    for l in levels:
        t = np.asarray(l).astype(np.float64)[..., :3]
        n = t.shape[1]
        y0, x0, face = (a.ravel() for a in np.meshgrid(np.arange(-1, n), np.arange(-1, n), np.arange(6), indexing="ij"))
        taps = []
        for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)):
            i, j = x0 + di, y0 + dj
            outside = (i < 0) | (i >= n) | (j < 0) | (j >= n)
            uc, vc = 2.0 * (i + 0.5) / n - 1.0, 2.0 * (j + 0.5) / n - 1.0
            f2, u2, v2 = cube_coord(cube_direction(face, uc, vc))
            i2 = np.clip(np.floor((u2 + 1.0) * 0.5 * n).astype(np.int64), 0, n - 1)
            j2 = np.clip(np.floor((v2 + 1.0) * 0.5 * n).astype(np.int64), 0, n - 1)
            taps.append(t[np.where(outside, f2, face), np.where(outside, j2, np.clip(j, 0, n - 1)), np.where(outside, i2, np.clip(i, 0, n - 1))])
        taps = np.stack(taps)
        worst = max(worst, float((taps.max(0) - taps.min(0)).max()))
    return worst


# ---- IBLResources.init in float64 ----

def _unit64(v):
    return v / np.sqrt((v * v).sum(-1))[..., None]


def sample_env_color64(d, roughness):
    """:106-121"""
    sky, ground = np.array([0.65, 0.72, 0.9]), np.array([0.12, 0.12, 0.14])
    t = np.clip(d[..., 1] * 0.5 + 0.5, 0.0, 1.0)
    color = ground + (sky - ground) * t[..., None]
    sun_dir = _unit64(np.array([0.2, 0.9, 0.1]))
    ndotl = np.maximum((d * sun_dir).sum(-1), 0.0)
    sun = np.power(ndotl, 800.0 + (30.0 - 800.0) * roughness) * 4.0
    return np.clip(color + sun[..., None], 0.0, 1.0)


def default_env64(size, mip_count, variant=None):
    """-> a list of [6][n][n][4] float64, one per level (:16-58)."""
    out = []
    for mip, n in enumerate(level_sizes(size, mip_count)):
        rough = mip / (mip_count - 1) if mip_count > 1 else 0.0
        c = 2.0 * (np.arange(n) + 0.5) / n - 1.0
        v, u = np.meshgrid(c, c, indexing="ij")
        level = np.ones((6, n, n, 4))
        for face in range(6):
            d = _unit64(cube_direction(np.full((n, n), face), u, v, flip_v=variant == "flip_v"))
            level[face, ..., :3] = sample_env_color64(d, rough)
        out.append(level)
    return out


def _radical_inverse(i):
    x = np.asarray(i, np.uint64) & 0xFFFFFFFF
    x = ((x << 16) | (x >> 16)) & 0xFFFFFFFF
    x = (((x & 0x55555555) << 1) | ((x & 0xAAAAAAAA) >> 1)) & 0xFFFFFFFF
    x = (((x & 0x33333333) << 2) | ((x & 0xCCCCCCCC) >> 2)) & 0xFFFFFFFF
    x = (((x & 0x0F0F0F0F) << 4) | ((x & 0xF0F0F0F0) >> 4)) & 0xFFFFFFFF
    x = (((x & 0x00FF00FF) << 8) | ((x & 0xFF00FF00) >> 8)) & 0xFFFFFFFF
    return x.astype(np.float64) * 2.3283064365386963e-10


def default_brdf_lut64(size, sample_count, variant=None, terms=False):
    """-> [size][size][2] float64 (:60-89, :123-175). terms=True: also the bar [size][size] of LUT_BAR below. Row y is roughness, column x is nDotV, both max(i / (size - 1), 0.001) (0.001 at size 1)."""
    with np.errstate(all="ignore"):
        axis = np.fmax(np.arange(size) / np.float64(size - 1), 0.001)
    rough = axis[:, None, None]
    ndv = (np.arange(size) / max(size - 1, 1) if variant == "unclamped_ndotv" else axis)[None, :, None]
    i = np.arange(sample_count)
    xi_x, xi_y = (i / sample_count)[None, None, :], _radical_inverse(i)[None, None, :]
    Vx, Vz = np.sqrt(np.maximum(1.0 - ndv * ndv, 0.0)), ndv
    a = rough * rough
    phi = 2.0 * np.pi * xi_x
    cos_t = np.sqrt((1.0 - xi_y) / (1.0 + (a * a - 1.0) * xi_y))
    sin_t = np.sqrt(np.maximum(1.0 - cos_t * cos_t, 0.0))
    Hx, Hy, Hz = np.cos(phi) * sin_t, np.sin(phi) * sin_t, cos_t
    vdh = Vx * Hx + Vz * Hz
    Lx, Ly, Lz = 2.0 * vdh * Hx - Vx, 2.0 * vdh * Hy, 2.0 * vdh * Hz - Vz
    with np.errstate(all="ignore"):
        Lz = Lz / np.sqrt(Lx * Lx + Ly * Ly + Lz * Lz)
    NoL, NoH, VoH = np.maximum(Lz, 0.0), np.maximum(Hz, 0.0), np.maximum(vdh, 0.0)
    k = (rough + 1.0) ** 2 / 8.0 if variant == "k_direct" else (rough * rough) * 0.5
    with np.errstate(all="ignore"):
        G = (ndv / (ndv * (1.0 - k) + k)) * (NoL / (NoL * (1.0 - k) + k))
        gvis = np.where(NoL > 0.0, (G * VoH) / np.maximum(NoH * ndv, 1e-4), 0.0)
    Fc = np.power(1.0 - VoH, 5.0)
    A, B = ((1.0 - Fc) * gvis).sum(-1) / sample_count, (Fc * gvis).sum(-1) / sample_count
    out = np.stack([B, A], -1) if variant == "swap_ab" else np.stack([A, B], -1)
    if not terms:
        return out
    # the bar of the module's LUT_BAR note, per entry
    den = np.maximum(NoH * ndv, 1e-4)
    gV = ndv / (ndv * (1.0 - k) + k)
    with np.errstate(all="ignore"):
        d_voh = np.where(NoL > 0.0, G / den + 5.0 * gvis, 0.0)
        d_nol = np.where(NoL > 0.0, (gV * VoH / den) * k / (NoL * (1.0 - k) + k) ** 2, 0.0)
    bar = U32 * (((sample_count - 1) + TERM_ROUNDINGS) * gvis.mean(-1) + ABSOLUTE_ROUNDINGS * (d_voh + d_nol).mean(-1))
    return out, bar


# LUT_BAR. The float32 builder against default_brdf_lut64, per entry, from the operation count of float32 arithmetic (u = 2**-24),
# to first order, in the manner of skin_ref:
#   the sum: sampleCount - 1 additions, each rounding a partial sum that is at most the sum of the terms' magnitudes; both A's and
#   B's terms are at most GVis: (sampleCount - 1) u mean(GVis);
#   a term: at most TERM_ROUNDINGS = 40 roundings deep (xi 1, phi 2, cos / sin of phi 2 at a libm's accuracy, cosTheta 5,
#   sinTheta 3, H 1, dot(V, H) 3, L 4, its normalisation 6, geometrySmith 8, GVis 3, Fc 2): 40 u GVis;
#   VoH = dot(V, H) and NoL = L.z are sums of products of components of unit vectors (L before normalisation has length at most 3):
#   their roundings are absolute, about ABSOLUTE_ROUNDINGS = 8 u, however small the value; the term turns them into
#   8 u (|dT/dVoH| + |dT/dNoL|) with dT/dVoH <= G / max(NoH nDotV, 1e-4) + 5 GVis (GVis itself and Fc = (1 - VoH)^5) and
#   dT/dNoL = gV VoH / max(NoH nDotV, 1e-4) * k / (NoL (1 - k) + k)^2 (through gL). At nDotV = 0.001 the division by
#   NoH nDotV makes this the largest part.
# Not counted: the cancellation in sinTheta^2 = 1 - cosTheta^2 at roughness 0.001, whose rigorous bound is too loose to be a check
# (sqrt(3 u) on sinTheta); the bar is tighter than a rigorous one there.
U32 = 2.0 ** -24
TERM_ROUNDINGS = 40
ABSOLUTE_ROUNDINGS = 8
