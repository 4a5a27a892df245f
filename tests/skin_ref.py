"""TEST INFRASTRUCTURE: the float64 reference of the 4-weight linear-blend skinning, its per-element error bars, and the
mesh / palette generators the skinning tests share (tests/test_skin_reference.py on the CPU, tests/test_gpu_skin_forms.py on the GPU).

The bars are derived from the operation count of float32 arithmetic, not fitted to any implementation. u = 2**-24 (the unit
roundoff of float32, half an ulp of 1).

Position. A skinned coordinate is  sum_j w_j * (sum_c M_j[r][c] * (p, 1)[c])  over the influences with w_j > 0. Every way the code
under test evaluates it is 8 roundings deep:
    the kernels   weight x matrix entry (1), three blend adds (3), blended entry x coordinate (1), three adds of the row sum (3);
    the oracle    matrix entry x coordinate (1), three adds of the row sum (3), x weight (1), three adds over the influences (3).
A rounding at depth k perturbs the result by at most u times the magnitude of the partial sum it rounds, and every partial sum is
bounded by
    mag[r] = sum_j w_j * sum_c |M_j[r][c]| * |(p, 1)[c]|
so |got - ref| <= ((1 + u)**8 - 1) * mag = 8 u mag + O(u**2). A fused multiply-add only removes roundings. The ninth unit
covers the second-order terms and the rounding of the float64 reference itself:
    |got - ref| <= 9 u mag                                                        per component.

Normal and tangent xyz. The blended, unnormalised vector N' carries the same 8 roundings with (n, 0) / (t.xyz, 0) in place of
(p, 1): |dN'| <= 9 u magN per component, so ||dN'||_2 <= 9 u ||magN||_2. Normalising divides by ||N||: the component of dN' along
N drops out and the rest is scaled, |d(N'/||N'||)| <= ||dN'||_2 / ||N||. The normalisation itself adds, relative to a component
of a unit vector (<= 1):
    sum of squares   3 u relative (three products and two adds of positive terms, at most 3 roundings deep), halved by the
                     inverse square root: 1.5 u, counted as 3 u
    inverse square root   2 u (one ulp of a result in [1, 2) for the hardware's single-precision instruction; a correctly rounded
                     1 / sqrt costs less)
    final multiply   1 u
together
    |got - ref| <= 9 u ||magN||_2 / ||N|| + 6 u                                     per component.
Tangent w is a copy (bit-equal); the fourth float of a padded16 position / normal is exactly 0.

In float32 numpy, in both evaluation orders, on 200,000 vertices at 65 and 256 bones the worst ratio of error to bar was 0.37 for
positions and 0.16 for directions; a wrong bone index or a dropped influence misses the bars by orders of magnitude."""
import numpy as np

U32 = 2.0 ** -24


def metal_skinning_f64(pos, nrm, tan, idx, w, palette, magnitudes=False):
    """skinningKernel, RayTracing.metalinc:758-775. palette: [B][16] column-major float4x4 (palette[b] * float4 = sum_c col_c * v_c).
    magnitudes=True adds a dict: mag / magN / magT [V][3] (sum_j w_j |M_j| . |v| over the influences with w_j > 0, for (p, 1),
    (n, 0), (t.xyz, 0)) and lenN / lenT [V], the lengths of the blended normal and tangent before normalisation."""
    M = palette.astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)  # [b][row][col]
    p4 = np.concatenate([pos, np.ones((len(pos), 1))], 1).astype(np.float64)
    n4 = np.concatenate([nrm, np.zeros((len(pos), 1))], 1).astype(np.float64)
    t4 = np.concatenate([tan[:, :3], np.zeros((len(pos), 1))], 1).astype(np.float64)
    acc, nacc, tacc = (np.zeros((len(pos), 3)) for _ in range(3))
    mags = [np.zeros((len(pos), 3)) for _ in range(3)] if magnitudes else None
    for j in range(4):
        wj = w[:, j].astype(np.float64)
        use = (wj > 0.0)[:, None]                                        # `if (w.x > 0.0)`
        Mj = M[idx[:, j]]
        acc += np.where(use, np.einsum("vrc,vc->vr", Mj, p4)[:, :3] * wj[:, None], 0.0)
        nacc += np.where(use, np.einsum("vrc,vc->vr", Mj, n4)[:, :3] * wj[:, None], 0.0)
        tacc += np.where(use, np.einsum("vrc,vc->vr", Mj, t4)[:, :3] * wj[:, None], 0.0)
        if magnitudes:
            Aj = np.abs(Mj)
            for m, v4 in zip(mags, (p4, n4, t4)):
                m += np.where(use, np.einsum("vrc,vc->vr", Aj, np.abs(v4))[:, :3] * wj[:, None], 0.0)
    nn = nacc / np.linalg.norm(nacc, axis=1, keepdims=True)
    tt = tacc / np.linalg.norm(tacc, axis=1, keepdims=True)
    out = (acc, nn, np.concatenate([tt, tan[:, 3:4].astype(np.float64)], 1))
    if not magnitudes:
        return out
    return out + ({"mag": mags[0], "magN": mags[1], "magT": mags[2], "lenN": np.linalg.norm(nacc, axis=1), "lenT": np.linalg.norm(tacc, axis=1)},)


def skin_reference(case, palettes):
    """The float64 reference of a crowd: palettes [chars][B][16] float32 (or [B][16] for one character) over the mesh dict `case`
    -> dict(pos [chars * V][3], nrm, tan [chars * V][4], posBar [.][3], nrmBar [.], tanBar [.]); the bars of the module docstring."""
    pal = np.asarray(palettes, np.float32)
    if pal.ndim == 2:
        pal = pal[None]
    chars, B = pal.shape[0], pal.shape[1]
    V = case["positions"].shape[0]
    assert int(case["boneIndices"].max()) < B
    tile = lambda a: np.tile(a, (chars, 1))
    idx = (case["boneIndices"].astype(np.int64)[None] + (np.arange(chars, dtype=np.int64) * B)[:, None, None]).reshape(chars * V, 4)
    p, n, t, m = metal_skinning_f64(tile(case["positions"]), tile(case["normals"]), tile(case["tangents"]), idx, tile(case["boneWeights"]),
                                    pal.reshape(chars * B, 16), magnitudes=True)
    assert np.isfinite(p).all() and np.isfinite(n).all() and np.isfinite(t).all()
    assert m["lenN"].min() > 0 and m["lenT"].min() > 0, "a blended normal or tangent of zero length has no direction to compare"
    return {"pos": p, "nrm": n, "tan": t, "posBar": 9 * U32 * m["mag"],
            "nrmBar": 9 * U32 * np.linalg.norm(m["magN"], axis=1) / m["lenN"] + 6 * U32,
            "tanBar": 9 * U32 * np.linalg.norm(m["magT"], axis=1) / m["lenT"] + 6 * U32}


def check_streams(got_pos, got_nrm, got_tan, ref, name, rows=None):
    """Every element of the three streams against the bars. got_pos / got_nrm [n][3 or 4] (a fourth float must be exactly 0),
    got_tan [n][4]; rows: the slice of the reference's vertices the streams hold. -> (worst position ratio, worst direction ratio)."""
    rows = slice(None) if rows is None else rows
    worst = []
    for g, r, bar, what in ((got_pos, ref["pos"][rows], ref["posBar"][rows], "position"),
                            (got_nrm, ref["nrm"][rows], ref["nrmBar"][rows][:, None], "normal"),
                            (got_tan, ref["tan"][rows][:, :3], ref["tanBar"][rows][:, None], "tangent")):
        g = np.asarray(g)
        assert g.shape[0] == r.shape[0], (name, what, g.shape, r.shape)
        assert np.isfinite(g).all(), (name, what, "not finite")
        err = np.abs(g[:, :3].astype(np.float64) - r)
        ratio = err / np.broadcast_to(bar, err.shape)
        worst.append(float(ratio.max()) if ratio.size else 0.0)
        if worst[-1] > 1.0:
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            raise AssertionError(f"{name}: {int((ratio > 1).sum())} of {ratio.size} {what} components beyond the bar; worst at vertex {i[0]} "
                                 f"component {i[1]}: got {g[i]!r} ref {r[i]!r} |d| {err[i]:.3g} bar {np.broadcast_to(bar, err.shape)[i]:.3g}")
        if what != "tangent" and g.shape[1] == 4:
            assert (g[:, 3] == 0).all(), (name, what, "padding float is not 0")
    assert np.array_equal(np.asarray(got_tan)[:, 3].astype(np.float64), ref["tan"][rows][:, 3]), (name, "tangent w is a copy")
    return worst[0], max(worst[1], worst[2])


def make_skin_case(V, B, seed):
    """A mesh dict for CharacterEngine.upload_skinned_mesh (tangents supplied: no uvs / indices needed) made to trip a skinning kernel:
    positions at the crowd's world scale (N(0, 1) x 50: rotation and translation terms both matter), unit normals, tangents with
    w = +-1; weights with 40 % zeros, a negative fourth weight on every 17th vertex, renormalised over the positive ones; and rows
    fixed by vertex index (v % 29): 3 = first weight exactly 0 with the later ones positive, 7 = all four influences on one bone,
    11 = bones 0 and B - 1 only, 13 = only the fourth weight positive."""
    rng = np.random.default_rng(seed)
    pos = (rng.normal(0, 1, (V, 3)) * 50.0).astype(np.float32)
    nrm = rng.normal(0, 1, (V, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    txyz = rng.normal(0, 1, (V, 3))
    txyz /= np.linalg.norm(txyz, axis=1, keepdims=True)
    tan = np.c_[txyz, rng.choice([-1.0, 1.0], V)].astype(np.float32)
    idx = rng.integers(0, B, (V, 4)).astype(np.uint16)
    wgt = rng.uniform(0, 1, (V, 4)).astype(np.float32)
    wgt[rng.uniform(size=(V, 4)) < 0.4] = 0
    wgt[:, 0] = np.maximum(wgt[:, 0], 0.05)
    wgt[::17, 3] = -0.25                                   # a negative weight is skipped like a zero one (`w > 0`)
    k = np.arange(V) % 29
    wgt[k == 3] = (0.0, 0.5, 0.3, 0.2)
    idx[k == 7] = idx[k == 7][:, :1]
    idx[k == 11] = (0, B - 1, 0, B - 1)
    wgt[k == 11] = (0.4, 0.3, 0.2, 0.1)
    wgt[k == 13] = (0.0, 0.0, 0.0, 1.0)
    wgt /= np.maximum(wgt, 0).sum(1, keepdims=True)
    assert np.isfinite(wgt).all() and (np.maximum(wgt, 0).sum(1) > 0.5).all()
    return {"positions": pos, "normals": nrm, "tangents": tan, "boneIndices": idx, "boneWeights": wgt.astype(np.float32)}


def rigid_shear_palette(B, rng, translation=0.5):
    """[B][16] column-major float32: a random rotation plus N(0, 0.02) shear per bone (what model * invBind looks like
    mid-animation), translations N(0, translation)."""
    pal = np.zeros((B, 4, 4), np.float64)
    for b in range(B):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        x, y, z, s = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s)],
                      [2 * (x * y + z * s), 1 - 2 * (x * x + z * z), 2 * (y * z - x * s)],
                      [2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)]])
        pal[b, :3, :3] = R + rng.normal(0, 0.02, (3, 3))
        pal[b, :3, 3] = rng.normal(0, translation, 3)
        pal[b, 3, 3] = 1.0
    return np.ascontiguousarray(pal.transpose(0, 2, 1).reshape(B, 16), np.float32)   # column-major
