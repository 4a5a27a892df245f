"""TEST INFRASTRUCTURE: the shaded frame (include/sge_amd_render.h) written from the Metal text (raytraceKernel,
RayTracing.metalinc:197-730, with frame.textureCount == 0 and eval_spec_ibl = 0), vectorised over pixels per stage. The intersector is
scene_ref.SceneRef.intersect: the CPU oracle's scan over every triangle.

Two ray-arithmetic paths and one shading path:
  path "A": every quantity that becomes a ray (the primary direction, hitPos, bias, origins, reflect and refract directions) is
            computed in numpy float32 in the order the header pins;
  path "B": the same expressions in float64, rounded to float32 only when handed to the scan.
Shading given the hits runs in `shade` = float64 (float32 gives the restatement whose distance from float64 sets the GPU test's
bar); hash12_rt always runs in float32 in the text's order.

Every stage of the frame issues its queries for all pixels at once and appends one (scene id, primitive) array to `trace`
(-2: the pixel did not issue this query, -1: a miss). The stages come in the order a pixel issues them, so two renders agree on a
pixel's queries, hits and branches exactly when their traces agree on that pixel: that is the *stable* pixel of the tests.
"""
import numpy as np

from scene_ref import STATIC_BASE

BG = (0.02, 0.02, 0.03)


def clamp_materials(materials):
    """sample_material's clamps (:143-150) on abi.render_material_dtype records."""
    m = np.array(materials, copy=True)
    m["alpha"] = np.clip(m["alpha"], 0, 1)
    m["metallic"] = np.clip(m["metallic"], 0, 1)
    m["roughness"] = np.clip(m["roughness"], np.float32(0.05), 1)
    m["occlusionStrength"] = np.clip(m["occlusionStrength"], 0, 1)
    m["transmission"] = np.clip(m["transmission"], 0, 1)
    m["ior"] = np.maximum(m["ior"], 1)
    return m


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def _sat(x):
    return np.minimum(np.maximum(x, 0), 1)


def hash12_rt(gx, gy):
    """:15-19 in float32, the text's order."""
    f = np.float32
    px, py = gx.astype(f), gy.astype(f)
    fract = lambda x: x - np.floor(x)
    p3 = np.stack([fract(px * f(0.1031)), fract(py * f(0.1031)), fract(px * f(0.1031))], -1)
    d = _dot(p3, np.stack([p3[..., 1] + f(33.33), p3[..., 2] + f(33.33), p3[..., 0] + f(33.33)], -1))
    p3 = p3 + d[..., None]
    return fract((p3[..., 0] + p3[..., 1]) * p3[..., 2])


def _fresnel(cos_theta, F0, st):
    p = np.power(_sat(st(1) - cos_theta), st(5))
    return F0 + (st(1) - F0) * p[..., None]


def _g1(nov, a, st):
    a2 = a * a
    denom = nov + np.sqrt(a2 + ((st(1) - a2) * nov) * nov)
    return (st(2) * nov) / np.maximum(denom, st(1e-4))


def eval_brdf(N, V, L, base, metallic, roughness, st):
    """:42-59"""
    nol, nov = _sat(_dot(N, L)), _sat(_dot(N, V))
    zero = (nol <= 0) | (nov <= 0)
    with np.errstate(all="ignore"):
        H = _unit(V + L)
        noh, voh = _sat(_dot(N, H)), _sat(_dot(V, H))
        alpha = roughness * roughness
        diff = (base * (st(1) - metallic)[..., None]) * (st(1) / st(3.14159265))
        a2 = alpha * alpha
        dd = (noh * noh) * (a2 - st(1)) + st(1)
        D = a2 / ((st(3.14159265) * dd) * dd)
        G = _g1(nov, alpha, st) * _g1(nol, alpha, st)
        F0 = st(0.04) + (base - st(0.04)) * metallic[..., None]
        F = _fresnel(voh, F0, st)
        spec = (F * (D * G)[..., None]) / np.maximum((st(4) * nov) * nol, st(1e-4))[..., None]
        out = diff + spec
    out[zero] = 0
    return out


def eval_env_sh(n, sh, st):
    """:65-86; sh [9][3]"""
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    c0, c1, c2, c3, c4 = st(0.282095), st(0.488603), st(1.092548), st(0.315392), st(0.546274)
    r = sh[0] * c0 + np.zeros(n.shape, st)
    r = r + sh[1] * (c1 * y)[..., None]
    r = r + sh[2] * (c1 * z)[..., None]
    r = r + sh[3] * (c1 * x)[..., None]
    r = r + sh[4] * ((c2 * x) * y)[..., None]
    r = r + sh[5] * ((c2 * y) * z)[..., None]
    r = r + sh[6] * (c3 * ((st(3) * z) * z - st(1)))[..., None]
    r = r + sh[7] * ((c2 * x) * z)[..., None]
    r = r + sh[8] * (c4 * (x * x - y * y))[..., None]
    return r


class RenderRef:
    """scene: a scene_ref.SceneRef; materials: abi.render_material_dtype records; static_materials [S] / crowd_materials [chars]
    (None: material 0); lights: abi.render_light_dtype records."""

    def __init__(self, scene, materials, static_materials, crowd_materials, lights):
        self.scene = scene
        self.mats = clamp_materials(materials)
        self.static_materials = None if static_materials is None else np.asarray(static_materials, np.int64)
        self.crowd_materials = None if crowd_materials is None else np.asarray(crowd_materials, np.int64)
        self.lights = np.asarray(lights)

    def _material_ids(self, inst):
        inst = np.asarray(inst, np.int64)
        out = np.zeros(len(inst), np.int64)
        st = inst >= STATIC_BASE
        if self.static_materials is not None:
            out[st] = self.static_materials[inst[st] - STATIC_BASE]
        if self.crowd_materials is not None:
            out[~st] = self.crowd_materials[np.maximum(inst[~st], 0)]
        return out

    def _query(self, R, idx, o, d, tmin, tmax):
        """One stage: the pixels `idx` issue a closest-hit query. Appends to the trace, counts, returns the records."""
        ids = np.full(R["n"], -2, np.int64)
        prims = np.full(R["n"], -2, np.int64)
        if len(idx):
            h = self.scene.intersect(np.ascontiguousarray(o, np.float32), np.ascontiguousarray(np.broadcast_to(d, o.shape), np.float32), -1,
                                     min_distance=np.ascontiguousarray(np.broadcast_to(tmin, (len(idx),)), np.float32),
                                     max_distance=np.ascontiguousarray(np.broadcast_to(tmax, (len(idx),)), np.float32))
            ids[idx] = np.where(h["hit"] == 1, h["instance"], -1)
            prims[idx] = np.where(h["hit"] == 1, h["primitive"], -1)
            R["queries"][idx] += 1
        else:
            h = np.zeros(0, [("hit", "<i4"), ("primitive", "<i4"), ("instance", "<i4"), ("distance", "<f4"), ("geomNormal", "<f4", 3)])
        R["trace"].append((ids, prims))
        return h

    def _surface(self, R, idx, o, d, h, phase):
        """The shading of one surface per pixel of idx (all hit): :247-380, :401-526, :572-695."""
        rt, st, cam = R["rt"], R["st"], R["cam"]
        k = len(idx)
        t = h["distance"].astype(rt)
        hit_pos = o + d * t[:, None]
        bias = np.maximum(rt(0.002), t * rt(0.002))
        N = h["geomNormal"].astype(rt)
        m = self.mats[self._material_ids(h["instance"])]
        V = _unit(-d)
        cam_dist = np.sqrt(_dot(hit_pos - cam, hit_pos - cam))
        Ns, Vs = N.astype(st), V.astype(st)
        base, metallic, rough = m["baseColor"].astype(st), m["metallic"].astype(st), m["roughness"].astype(st)
        direct = np.zeros((k, 3), st)
        shadow0 = np.ones(k, st)
        for i in range(R["nlights"]):
            l = self.lights[i]
            if l["enabled"] < 0.5:
                continue
            max_dist = rt(l["maxDistance"]) if l["maxDistance"] > 0 else rt(1e6)
            L = _unit(-l["direction"].astype(rt))
            ndotl = np.maximum(_dot(N, L), rt(0))
            act = ~(cam_dist > max_dist) & (ndotl > 0)
            shadow = np.ones(k, st)
            if i == 0 or phase == 2:
                so = hit_pos + N * bias[:, None]
                smin = bias * rt(0.5)
                alive = act.copy()
                for _ in range(4):
                    sel = np.flatnonzero(alive)
                    hh = self._query(R, idx[sel], so[sel], L, smin[sel], max_dist)
                    hm = hh["hit"] == 1
                    on = sel[hm]
                    shadow[on] = shadow[on] * (st(1) - self.mats["alpha"][self._material_ids(hh["instance"][hm])].astype(st))
                    so[on] = (so[on] + L * hh["distance"][hm].astype(rt)[:, None]) + (L * bias[on][:, None]) * rt(2)
                    smin[on] = rt(0.001)
                    alive[sel[~hm]] = False
                    alive &= shadow > st(0.02)
            Ls = np.broadcast_to(L.astype(st), (k, 3))
            brdf = eval_brdf(Ns, Vs, Ls, base, metallic, rough, st)
            Li = l["color"].astype(st) * st(l["intensity"])
            direct[act] += ((brdf * Li) * (ndotl.astype(st) * shadow)[:, None])[act]
            if i == 0:
                shadow0 = np.where(act, shadow, st(1))
        ambient = ((base * eval_env_sh(Ns, R["sh"], st)) * R["ambient"]) * m["occlusionStrength"].astype(st)[:, None]
        color = (direct + ambient) + m["emissive"].astype(st)
        return {"hitPos": hit_pos, "bias": bias, "N": N, "V": V, "m": m, "color": color, "shadow0": shadow0}

    def render(self, frame, path="A", shade=np.float64):
        f = np.asarray(frame).reshape(-1)[0]
        rt = np.float32 if path == "A" else np.float64
        st = shade
        W, H = int(f["width"]), int(f["height"])
        n = W * H
        cam = f["cameraPosition"].astype(rt)
        R = {"n": n, "rt": rt, "st": st, "cam": cam, "nlights": int(f["dirLightCount"]), "sh": f["envSH"].astype(st),
             "ambient": st(f["ambientIntensity"]), "trace": [], "queries": np.zeros(n, np.int64)}
        gy, gx = np.divmod(np.arange(n), W)
        # the camera ray, :225-235
        px, py = (gx.astype(rt) + rt(0.5)) / rt(W), (gy.astype(rt) + rt(0.5)) / rt(H)
        nx, ny = px * rt(2) - rt(1), (rt(1) - py) * rt(2) - rt(1)
        M = f["invViewProj"].astype(rt).reshape(4, 4)  # M[c] is column c
        world = ((M[0] * nx[:, None] + M[1] * ny[:, None]) + M[2] * rt(1)) + M[3] * rt(1)
        d = _unit(world[:, :3] / world[:, 3:4] - cam)
        o = np.tile(cam, (n, 1))
        tmin = np.full(n, 0.001, rt)

        accum, accum_alpha = np.zeros((n, 3), st), np.zeros(n, st)
        layers, flags = np.zeros(n, np.int32), np.zeros(n, np.int32)
        a_inst, a_prim = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        a_dist, a_shadow = np.zeros(n, np.float32), np.ones(n, st)
        active = np.ones(n, bool)
        bg = np.array(BG, st)
        for layer in range(3):
            active &= accum_alpha < st(0.99)
            idx = np.flatnonzero(active)
            h = self._query(R, idx, o[idx], d[idx], tmin[idx], rt(1e6))
            hm = h["hit"] == 1
            active[idx[~hm]] = False
            idx, h = idx[hm], h[hm]
            S = self._surface(R, idx, o[idx], d[idx], h, 0)
            hit_pos, bias, N, V, m, color = S["hitPos"], S["bias"], S["N"], S["V"], S["m"], S["color"]
            dd = d[idx]
            if layer == 0:
                a_inst[idx], a_prim[idx], a_dist[idx], a_shadow[idx] = h["instance"], h["primitive"], h["distance"], S["shadow0"]
            base = m["baseColor"].astype(st)
            nov = _sat(_dot(N.astype(st), V.astype(st)))
            # the mirror path, :383-542
            j = np.flatnonzero((m["roughness"] <= np.float32(0.08)) & (m["metallic"] >= np.float32(0.8)))
            if layer == 0:
                flags[idx[j]] |= 1
            Rd = dd[j] - N[j] * (rt(2) * _dot(N[j], dd[j]))[:, None]
            ro = hit_pos[j] + N[j] * bias[j][:, None]
            rh = self._query(R, idx[j], ro, Rd, bias[j] * rt(0.5), rt(1e6))
            jh = rh["hit"] == 1
            RS = self._surface(R, idx[j][jh], ro[jh], Rd[jh], rh[jh], 1)
            racc, ralpha = np.zeros((len(j), 3), st), np.zeros(len(j), st)
            ralpha[jh] = RS["m"]["alpha"].astype(st)
            racc[jh] = RS["color"] * ralpha[jh][:, None]
            refl = racc + bg * (st(1) - ralpha)[:, None]
            F0 = st(0.04) + (base[j] - st(0.04)) * m["metallic"][j].astype(st)[:, None]
            Fm = _fresnel(nov[j], F0, st)
            color[j] = color[j] + (refl - color[j]) * Fm
            # the refraction path, :545-713
            ior = m["ior"].astype(rt)
            with np.errstate(all="ignore"):
                eta = rt(1) / ior
                flip = _dot(N, V) < 0
                nn = np.where(flip[:, None], -N, N)
                eta = np.where(flip, ior, eta)
                I = -V
                dn = _dot(nn, I)
                kk = rt(1) - (eta * eta) * (rt(1) - dn * dn)
                T = np.where((kk < 0)[:, None], rt(0), I * eta[:, None] - nn * (eta * dn + np.sqrt(np.maximum(kk, 0)))[:, None])
                go = (m["transmission"] > np.float32(0.001)) & (np.sqrt(_dot(T, T)) > 0)
            j = np.flatnonzero(go)
            if layer == 0:
                flags[idx[j]] |= 2
            with np.errstate(all="ignore"):
                Td = _unit(T[j])
            to = hit_pos[j] + T[j] * bias[j][:, None]
            th = self._query(R, idx[j], to, Td, bias[j] * rt(0.5), rt(1e6))
            jh = th["hit"] == 1
            TS = self._surface(R, idx[j][jh], to[jh], Td[jh], th[jh], 2)
            tacc, talpha = np.zeros((len(j), 3), st), np.zeros(len(j), st)
            talpha[jh] = TS["m"]["alpha"].astype(st)
            tacc[jh] = TS["color"] * talpha[jh][:, None]
            refr_bg = eval_env_sh(Td.astype(st), R["sh"], st) * R["ambient"]
            refr = tacc + refr_bg * (st(1) - talpha)[:, None]
            Fr = _fresnel(nov[j], np.full((len(j), 3), 0.04, st), st)
            trans = refr * base[j]
            mixc = trans * (st(1) - Fr) + color[j] * Fr
            color[j] = color[j] + (mixc - color[j]) * m["transmission"][j].astype(st)[:, None]
            # compositing, :715-721
            alpha = m["alpha"].astype(st)
            one_minus = st(1) - accum_alpha[idx]
            accum[idx] += (color * alpha[:, None]) * one_minus[:, None]
            accum_alpha[idx] += alpha * one_minus
            layers[idx] += 1
            o[idx] = hit_pos + dd * (bias * rt(2))[:, None]
            tmin[idx] = rt(0.001)
        out = accum + bg * (st(1) - accum_alpha)[:, None]
        dither = (hash12_rt(gx, gy) - np.float32(0.5)) * (np.float32(1.0) / np.float32(255.0))
        rgb = np.maximum(out + dither.astype(st)[:, None], 0)
        return {"rgb": rgb.reshape(H, W, 3), "layers": layers.reshape(H, W), "instance": a_inst.reshape(H, W), "primitive": a_prim.reshape(H, W),
                "distance": a_dist.reshape(H, W), "shadow": a_shadow.reshape(H, W), "alpha": accum_alpha.reshape(H, W),
                "queries": R["queries"].reshape(H, W), "flags": flags.reshape(H, W), "trace": R["trace"], "dir": d.astype(np.float32)}


def stable_pixels(a, b):
    """[H][W] bool: the two renders issued the same queries, got the same (scene id, primitive) from each and took the same branches."""
    assert len(a["trace"]) == len(b["trace"])
    ok = np.ones(a["queries"].size, bool)
    for (ia, pa), (ib, pb) in zip(a["trace"], b["trace"]):
        ok &= (ia == ib) & (pa == pb)
    ok &= (a["queries"].ravel() == b["queries"].ravel()) & (a["layers"].ravel() == b["layers"].ravel()) & (a["flags"].ravel() == b["flags"].ravel())
    return ok.reshape(a["queries"].shape)
