"""TEST INFRASTRUCTURE: textures in the shaded frame (include/sge_amd_render_textures.h) written from the Metal text: the bilinear
sampler of `constexpr sampler(mip_filter::linear, mag_filter::linear, min_filter::linear)` in a compute kernel (level 0, normalised
coordinates, clamp-to-edge), in numpy float32 in the order the header pins and in float64; and TexRenderRef, a render_ref.RenderRef
whose surface applies sample_material (RayTracing.metalinc:132-176), sample_alpha (:178-195) and the normal map (:283-316) from the
uv / normal / tangent / bitangent that scene_ref.SceneRef.intersect returns.

Precision follows render_ref: what becomes a ray (the mapped normal) is computed in the ray type of the path (A: float32 in the
pinned order, B: float64), what only shades (sample_material, sample_alpha) in the shading type.

Sampled values feed thresholds (roughness <= 0.08, metallic >= 0.8, accumAlpha < 0.99, shadow > 0.02, NdotL > 0, the flip of the
mapped N). The reference records per pixel the smallest distance of such a value from its threshold (`margin`); tex_stable_pixels
counts a pixel closer than a given term as unstable.

`variant` selects a deliberately wrong restatement (test_render_tex_reference.py shows that each misses the frame bar):
"no_offset" (no -0.5 texel offset), "wrap" (repeat addressing), "filter_first" (filtering before the sRGB decode), "flip_y" (the
normal map's y negated), "opaque_shadow" (sample_alpha ignoring the texture)."""
import numpy as np

from render_ref import RenderRef, _dot, _sat, _unit, eval_brdf, eval_env_sh, stable_pixels

TEXTURE_FIELDS = ("baseColor", "normal", "metallicRoughness", "emissive", "occlusion")


def srgb_table64():
    s = np.arange(256, dtype=np.float64) / 255.0
    return np.where(s <= 0.04045, s / 12.92, np.power((s + 0.055) / 1.055, 2.4))


def _decode(texels, srgb, table, ft):
    """uint8 [..., 4] -> ft [..., 4]: unorm, colour channels through the table for an sRGB texture."""
    out = texels.astype(ft) / ft(255.0)
    if srgb:
        out[..., :3] = np.asarray(table, ft)[texels[..., :3]]
    return out


def sample(rgba, srgb, uvs, ft=np.float32, table=None, variant=None):
    """The pinned sampler. rgba uint8 [H][W][4]; uvs [n][2]; ft float32 (the header's order, the device's table if given) or
    float64 (the formula's table) -> ft [n][4]."""
    rgba = np.asarray(rgba, np.uint8)
    H, W = rgba.shape[:2]
    if table is None:
        table = srgb_table64() if ft is np.float64 else srgb_table64().astype(np.float32)
    uv = np.asarray(uvs, ft).reshape(-1, 2)
    off = ft(0.0) if variant == "no_offset" else ft(0.5)
    with np.errstate(all="ignore"):
        def axis(c, size):
            if variant == "wrap":
                x = c * ft(size) - off
                x0 = np.floor(x)
                f = (x - x0).astype(ft)
                i0 = np.mod(x0.astype(np.int64), size)
                return i0, np.mod(i0 + 1, size), f
            x = np.fmin(np.fmax(c * ft(size) - off, ft(0.0)), ft(size - 1))
            i0 = np.floor(x).astype(np.int64)
            return i0, np.minimum(i0 + 1, size - 1), (x - i0.astype(ft)).astype(ft)
        x0, x1, fx = axis(uv[:, 0], W)
        y0, y1, fy = axis(uv[:, 1], H)
    fx, fy = fx[:, None], fy[:, None]
    one = ft(1.0)
    if variant == "filter_first":
        raw = [rgba[y, x].astype(ft) for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
        top = raw[0] * (one - fx) + raw[1] * fx
        bot = raw[2] * (one - fx) + raw[3] * fx
        mixed = top * (one - fy) + bot * fy
        out = mixed / ft(255.0)
        if srgb:
            s = out[:, :3].astype(np.float64)
            out[:, :3] = np.where(s <= 0.04045, s / 12.92, np.power((s + 0.055) / 1.055, 2.4)).astype(ft)
        return out
    t00, t10 = _decode(rgba[y0, x0], srgb, table, ft), _decode(rgba[y0, x1], srgb, table, ft)
    t01, t11 = _decode(rgba[y1, x0], srgb, table, ft), _decode(rgba[y1, x1], srgb, table, ft)
    top = t00 * (one - fx) + t10 * fx
    bot = t01 * (one - fx) + t11 * fx
    return top * (one - fy) + bot * fy


def adjacent_step(rgba, srgb):
    """The largest difference between decoded texels that a bilinear footprint joins (horizontal, vertical, diagonal)."""
    t = _decode(np.asarray(rgba, np.uint8), srgb, srgb_table64(), np.float64)
    d = [0.0]
    if t.shape[1] > 1:
        d.append(np.abs(t[:, 1:] - t[:, :-1]).max())
    if t.shape[0] > 1:
        d.append(np.abs(t[1:] - t[:-1]).max())
    if t.shape[0] > 1 and t.shape[1] > 1:
        d.append(np.abs(t[1:, 1:] - t[:-1, :-1]).max())
        d.append(np.abs(t[1:, :-1] - t[:-1, 1:]).max())
    return float(max(d))


def value_term(textures, uv_bar=1e-6, gains=None):
    """How far a sampled value may move when the uv moves by the uv bar of scene_ref.assert_records_match: a bilinear filter is
    continuous and piecewise linear, with slope at most (dimension) x (largest step between adjacent decoded texels) per unit uv
    along each axis; both axes may move. gains: {slot: the factor the slot's samples are multiplied by where they are used}."""
    gains = gains or {}
    return uv_bar * max([2 * max(t.shape[0], t.shape[1]) * adjacent_step(t, s) * gains.get(slot, 1.0) for slot, (t, s) in textures.items()] + [0.0])


def resolve_bindings(bindings, textures, count):
    """abi.render_material_textures_dtype records for materials [0, len(bindings)) -> [count] records whose indices name a texture
    that exists, or -1 (an index < 0, >= 32 or of an empty slot means no texture)."""
    out = np.zeros(count, np.asarray(bindings).dtype)
    for f in TEXTURE_FIELDS:
        out[f] = -1
    out["normalScale"] = 1.0
    b = np.asarray(bindings).reshape(-1)
    out[:len(b)] = b
    for f in TEXTURE_FIELDS:
        ok = np.isin(out[f], [s for s in textures if 0 <= s < 32])
        out[f][~ok] = -1
    return out


class TexRenderRef(RenderRef):
    """textures: {slot: (uint8 [H][W][4], srgb)}; bindings: abi.render_material_textures_dtype records for materials [0, len)."""

    def __init__(self, scene, materials, static_materials, crowd_materials, lights, textures=None, bindings=None, variant=None, table32=None):
        super().__init__(scene, materials, static_materials, crowd_materials, lights)
        self.textures = dict(textures or {})
        self.variant = variant
        self.table32 = table32  # the device's table when the test has it, else the formula's rounded to float32
        self.bind = None if bindings is None else resolve_bindings(bindings, self.textures, len(self.mats))
        self._margin = None

    def _sample(self, slots, uv, ft):
        """[k] slot per row (-1: none) -> ([k][4] ft, [k] bool sampled)."""
        out = np.ones((len(slots), 4), ft)
        for s in np.unique(slots[slots >= 0]):
            sel = slots == s
            rgba, srgb = self.textures[int(s)]
            out[sel] = sample(rgba, srgb, uv[sel], ft, self.table32 if ft is np.float32 else None,
                              self.variant if self.variant in ("no_offset", "wrap", "filter_first") else None)
        return out, slots >= 0

    def _note(self, R, idx, distance):
        m = R.setdefault("margin", np.full(R["n"], np.inf))
        m[idx] = np.minimum(m[idx], distance)
        self._margin = m

    def _surface(self, R, idx, o, d, h, phase):
        if self.bind is None:
            return super()._surface(R, idx, o, d, h, phase)
        rt, st, cam = R["rt"], R["st"], R["cam"]
        k = len(idx)
        t = h["distance"].astype(rt)
        hit_pos = o + d * t[:, None]
        bias = np.maximum(rt(0.002), t * rt(0.002))
        N = h["geomNormal"].astype(rt)
        ids = self._material_ids(h["instance"])
        src = self.mats[ids]
        m = np.zeros(k, [(name, st, src.dtype[name].shape) for name in src.dtype.names])
        for name in src.dtype.names:
            m[name] = src[name]
        V = _unit(-d)
        if k:
            b = self.bind[ids]
            uv = h["uv"]
            # sample_material, :152-174
            c, on = self._sample(b["baseColor"], uv, st)
            m["baseColor"] = m["baseColor"] * c[:, :3]
            m["alpha"] = m["alpha"] * c[:, 3]
            c, _ = self._sample(b["metallicRoughness"], uv, st)
            m["roughness"] = m["roughness"] * c[:, 1]
            m["metallic"] = m["metallic"] * c[:, 2]
            c, _ = self._sample(b["emissive"], uv, st)
            m["emissive"] = m["emissive"] * c[:, :3]
            c, _ = self._sample(b["occlusion"], uv, st)
            m["occlusionStrength"] = m["occlusionStrength"] * c[:, 0]
            # the normal map, :283-316
            c, on = self._sample(b["normal"], uv, rt)
            if on.any():
                n_tex = c[:, :3] * rt(2) - rt(1)
                if self.variant == "flip_y":
                    n_tex[:, 1] = -n_tex[:, 1]
                nov = _sat(_dot(N, V))
                s = _sat((nov - rt(0.05)) / (rt(0.5) - rt(0.05)))
                graze = (s * s) * (rt(3) - rt(2) * s)
                ns = rt(4) + np.maximum(b["normalScale"].astype(rt) - rt(4), rt(0)) * rt(0.25)
                x, y = n_tex[:, 0] * (ns * graze), n_tex[:, 1] * (ns * graze)
                z = np.sqrt(np.maximum(rt(1) - (x * x + y * y), rt(0)))
                nW, tW, bW = h["normal"].astype(rt), h["tangent"].astype(rt), h["bitangent"].astype(rt)
                with np.errstate(all="ignore"):
                    mapped = _unit((tW * x[:, None] + bW * y[:, None]) + nW * z[:, None])
                side = _dot(mapped, d)
                mapped = np.where((side > 0)[:, None], -mapped, mapped)
                N = np.where(on[:, None], mapped, N).astype(rt)
                self._note(R, idx[on], np.abs(side[on]).astype(np.float64))
            if phase == 0:
                self._note(R, idx, np.minimum(np.abs(m["roughness"] - 0.08), np.abs(m["metallic"] - 0.8)).astype(np.float64))
                acc = R.setdefault("accA", np.zeros(R["n"]))
                acc[idx] = acc[idx] + m["alpha"].astype(np.float64) * (1.0 - acc[idx])
                self._note(R, idx, np.abs(acc[idx] - 0.99))
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
            raw = _dot(N, L)
            ndotl = np.maximum(raw, rt(0))
            near = ~(cam_dist > max_dist)
            act = near & (ndotl > 0)
            shadow = np.ones(k, st)
            if i == 0 or phase == 2:
                if k:
                    mapped_here = self.bind[ids]["normal"] >= 0
                    sel = near & mapped_here
                    self._note(R, idx[sel], np.abs(raw[sel]).astype(np.float64))  # decides whether the shadow ray is shot
                so = hit_pos + N * bias[:, None]
                smin = bias * rt(0.5)
                alive = act.copy()
                for _ in range(4):
                    sel = np.flatnonzero(alive)
                    hh = self._query(R, idx[sel], so[sel], L, smin[sel], max_dist)
                    hm = hh["hit"] == 1
                    on = sel[hm]
                    shadow[on] = shadow[on] * (st(1) - self._alpha(hh[hm], st))
                    self._note(R, idx[on], np.abs(shadow[on].astype(np.float64) - 0.02))
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

    def _alpha(self, hh, st):
        """sample_alpha, :178-195, of the occluders hh."""
        ids = self._material_ids(hh["instance"])
        alpha = self.mats["alpha"][ids].astype(st)
        if len(ids) and self.variant != "opaque_shadow":
            c, on = self._sample(self.bind[ids]["baseColor"], hh["uv"], st)
            alpha = alpha * c[:, 3]
        return alpha

    def render(self, frame, path="A", shade=np.float64):
        self._margin = None
        out = super().render(frame, path, shade)
        shape = out["layers"].shape
        out["margin"] = np.full(shape, np.inf) if self._margin is None else self._margin.reshape(shape)
        return out


def tex_stable_pixels(a, b, term):
    """render_ref.stable_pixels, and no sampled value of either render within `term` of a threshold it feeds."""
    return stable_pixels(a, b) & (a["margin"] >= term) & (b["margin"] >= term)
