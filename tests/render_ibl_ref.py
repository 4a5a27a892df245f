"""TEST INFRASTRUCTURE: the shaded frame with specular IBL (include/sge_amd_render_ibl.h): IblRenderRef, a
render_tex_ref.TexRenderRef whose layer surfaces (phase 0 only; the bounce surfaces of :525-530 and :694-699 have no such term) add
eval_spec_ibl(...) * occlusion (RayTracing.metalinc:379-380) through ibl_ref, from the surface the base class shaded: the
normal-mapped N and the sampled roughness, metallic, base colour and occlusion when textures are bound. The term is shading: it runs
in the shading type, in the header's order ((direct + ambient) + spec * occlusion) + emissive: the base class shades the surface
with the emissive factors set to zero, which leaves direct + ambient exactly, and the emissive term (the factor times the emissive
texture's sample, as the base class has it) is added here behind the term.

The term feeds no threshold. What it adds to instability is the face selection of R: the reference records, per pixel, the smallest
ibl_ref.tie_margin of an R it sampled (`ibl_margin`)."""
import numpy as np

import ibl_ref as ir
from render_tex_ref import TexRenderRef, tex_stable_pixels


class IblRenderRef(TexRenderRef):
    """levels: ibl_ref.split_levels of the uploaded cube (float16); lut: float32 [H][W][4]. Either None: no term."""

    def __init__(self, *args, levels=None, lut=None, ibl_variant=None, **kw):
        super().__init__(*args, **kw)
        self.levels, self.lut, self.ibl_variant = levels, lut, ibl_variant
        self._ibl_margin = None
        self.spec_worst = 0.0  # the largest F0 * brdf.x + brdf.y met (the gain of a prefiltered value on its way into rgb)

    def _surface(self, R, idx, o, d, h, phase):
        st = R["st"]
        saved = self.mats
        self.mats = saved.copy()
        self.mats["emissive"] = 0
        try:
            S = super()._surface(R, idx, o, d, h, phase)  # colour = (direct + ambient) + 0
        finally:
            self.mats = saved
        ids = self._material_ids(h["instance"])
        emissive = saved["emissive"][ids].astype(st)
        if self.bind is not None and len(idx):
            c, _ = self._sample(self.bind[ids]["emissive"], h["uv"], st)
            emissive = emissive * c[:, :3]
        m = S["m"]
        if phase != 0 or self.levels is None or self.lut is None or not len(idx):
            S["color"] = S["color"] + emissive
            return S
        N, V = S["N"].astype(st), S["V"].astype(st)
        spec = ir.eval_spec_ibl(self.levels, self.lut, N, V, m["roughness"].astype(st), m["metallic"].astype(st), m["baseColor"].astype(st), st,
                                self.ibl_variant)
        S["color"] = (S["color"] + spec * m["occlusionStrength"].astype(st)[:, None]) + emissive
        if self._ibl_margin is None:
            self._ibl_margin = np.full(R["n"], np.inf)
        self._ibl_margin[idx] = np.minimum(self._ibl_margin[idx], ir.tie_margin(ir.reflect_dir(N, V)))
        brdf = ir.lut_sample(self.lut, np.stack([np.clip((N * V).sum(-1), 0, 1), m["roughness"].astype(st)], -1), np.float64)
        F0 = 0.04 + (m["baseColor"].astype(np.float64) - 0.04) * m["metallic"].astype(np.float64)[:, None]
        self.spec_worst = max(self.spec_worst, float((F0 * brdf[:, :1] + brdf[:, 1:2]).max()))
        return S

    def render(self, frame, path="A", shade=np.float64):
        self._ibl_margin = None
        out = super().render(frame, path, shade)
        shape = out["layers"].shape
        out["ibl_margin"] = np.full(shape, np.inf) if self._ibl_margin is None else self._ibl_margin.reshape(shape)
        return out


# The coordinate bar of R through the face projection. R = I - N * (2 * dot(N, I)) from unit vectors held to 1e-6 per component by
# the scene tests (scene_ref.assert_records_match's bar on the hit record's vectors): each component of R moves by at most
# (1 + 2 + 2 + 2) x 1e-6 (I itself, and N and I in each of the two places they enter the product, to first order), and u = a / b with
# |a| <= |b| moves by at most twice that relative to the face's major component.
R_COORD_BAR = 2 * 7e-6


def ibl_stable_pixels(a, b, term):
    """render_tex_ref.tex_stable_pixels, and no R of either render within R_COORD_BAR of a tie of the face selection."""
    return tex_stable_pixels(a, b, term) & (a["ibl_margin"] >= R_COORD_BAR) & (b["ibl_margin"] >= R_COORD_BAR)


def ibl_colour_term(levels, size, spec_worst):
    """What R_COORD_BAR may move the term by on its way into rgb: a bilinear filter is piecewise linear in the texel coordinate
    ((u + 1) / 2 * n: slope n / 2 per unit u, both axes), between texels at most ibl_ref.adjacent_step apart, at the levels used; times
    the largest F0 * brdf.x + brdf.y; occlusion, alpha and the compositing weights are at most 1."""
    return R_COORD_BAR * size * ir.adjacent_step(levels) * spec_worst
