"""Diagnostic: rays/s of the ray scene (include/sge_amd_ray_scene.h) on one MI355X, rays and results resident on the device.

The settled 10,000-character crowd of tools/ray_bench.py, plus the 17-Cheese render mesh as one static instance and 1,000
instances of a small box. One process; the two forms of each comparison alternate A/B five times each, every launch timed with HIP
events on the context's stream after a warm-up launch of both.
  (a) crowd only: sge_scene_intersect_device with an empty static list against sge_blas_intersect_device(any_instance = 1), the
      reference; the scene form should sit within the spread of the reference's own five runs
  (b) whole-scene closest hit, rays/s
  (c) occlusion on the same rays; it does a subset of (b)'s work and must not be slower
With --variants, behind those lines and in the same process: (b) and (c) again, on the same rays and statics, for the crowd with three
mesh variants chosen by sge_lod_select (tools/variant_crowd.py) — first the control, whose variants all hold the full mesh (the
ragged kernels over the uniform crowd's geometry: the price of the per-character table walk alone, read against the uniform lines
above), then full / half / quarter vertex count.
usage: scene_ray_bench.py [--chars N] [--rays M] [--boxes K] [--variants] [--out FILE]"""
import importlib, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sge = importlib.import_module("swift-game-engine_amd")
abi = sge.abi
import torch

arg = lambda k, d, cast=int: cast(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
n, m, boxes = arg("--chars", 10000), arg("--rays", 200000), arg("--boxes", 1000)
out_path = arg("--out", None, str)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def flat_normals(pos, idx):
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    fn = np.cross(pos[tri[:, 1]] - pos[tri[:, 0]], pos[tri[:, 2]] - pos[tri[:, 0]]).astype(np.float64)
    nrm = np.zeros(pos.shape, np.float64)
    for k in range(3):
        np.add.at(nrm, tri[:, k], fn)
    length = np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.where(length > 0, nrm / np.maximum(length, 1e-30), (0.0, 1.0, 0.0)).astype(np.float32)


def upload_mesh(eng, mesh, pos, idx):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
    return eng.scene_mesh_upload(mesh, pos, flat_normals(pos, idx), np.tile(np.array([1, 0, 0, 1], np.float32), (len(pos), 1)), idx)


eng = sge.CharacterEngine(0)
ybot = sge.assets.YBotAssets()
sge.crowd.upload_character_assets(eng, ybot)
terrain = sge.crowd.upload_terrain(eng)
sge.crowd.spawn_crowd(eng, ybot, n, terrain, mode="ccd")
eng.blas_build(eng.mesh["indices"])
for _ in range(130):
    eng.tick(stages=abi.STAGE_ALL | abi.STAGE_BLAS_REFIT)
b = eng.download(what=("bodies",))["bodies"]
P = b["position"].astype(np.float32)
mats = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
mats[:, 3, :3] = P                                            # column-major: translation in the last column
eng.blas_instances(mats.reshape(n, 16))

# statics: the cheese, scaled to a sixth of the crowd's extent and set down in its middle; small boxes scattered over it
cheese = sge.crowd._load_static_parts("cheese")[0]
cpos = np.asarray(cheese["positions"], np.float32).reshape(-1, 3)
info = upload_mesh(eng, 0, cpos, cheese["indices"])
s = np.float32(8.0)
bp = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
bi = np.array([0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3], np.uint32)
upload_mesh(eng, 1, bp, bi)
rng = np.random.default_rng(1)
lo, hi = P.min(0), P.max(0)
scale = np.float32((hi - lo)[[0, 2]].max() / 6 / max(np.ptp(cpos, axis=0).max(), 1e-6))
S = np.tile(np.eye(4, dtype=np.float32), (1 + boxes, 1, 1))
S[0, :3, :3] *= scale
S[0, 3, :3] = (lo + hi) / 2 - scale * (cpos.min(0) + cpos.max(0)) / 2 * (1, 0, 1) - (0, scale * cpos[:, 1].min(), 0)
S[1:, 3, :3] = np.stack([rng.uniform(lo[0], hi[0], boxes), rng.uniform(lo[1], hi[1], boxes) + 1.0, rng.uniform(lo[2], hi[2], boxes)], 1)
mesh_of = np.array([0] + [1] * boxes, np.int32)

inst = rng.integers(0, n, m)
target = P[inst] + rng.uniform(-0.6, 0.6, (m, 3)).astype(np.float32) * (1, 2, 1)
origin = target + (rng.normal(size=(m, 3)) * (8, 2, 8) + (0, 6, 0)).astype(np.float32)
d = target - origin
d /= np.linalg.norm(d, axis=1, keepdims=True)
r = np.zeros(m, abi.blas_ray_dtype)
r["origin"], r["direction"], r["minDistance"], r["maxDistance"], r["instance"] = origin, d, 0.001, 1e6, -1
d_r = torch.from_numpy(r.view(np.uint8).copy()).to("cuda:0")
d_h = torch.zeros(m * abi.blas_hit_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
d_o = torch.zeros(m, dtype=torch.int32, device="cuda:0")
torch.cuda.synchronize()
stream = torch.cuda.ExternalStream(eng.stream_handle(), device="cuda:0")



def forms_of(e):
    return {"blas_intersect_device": lambda: e.blas_intersect_device(d_r.data_ptr(), m, d_h.data_ptr()),
            "scene_intersect_device": lambda: e.scene_intersect_device(d_r.data_ptr(), m, d_h.data_ptr()),
            "scene_occluded_device": lambda: e.scene_occluded_device(d_r.data_ptr(), m, d_o.data_ptr())}


forms = forms_of(eng)


def alternate(a, b, rounds=5):
    """ms of every launch of forms a and b, alternating, after one warm-up launch of each."""
    for k in (a, b):
        forms[k]()
    eng.synchronize()
    ms = {a: [], b: []}
    for _ in range(rounds):
        for k in (a, b):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            forms[k]()
            e1.record(stream)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def report(label, ms):
    v = np.array(ms)
    say("  %-24s %s ms  median %.3f  min %.3f  max %.3f  = %.1f M rays/s" % (label, " ".join("%.3f" % x for x in v), np.median(v), v.min(), v.max(), m / np.median(v) / 1e3))
    return v


say("scene_ray_bench: %d characters, %d rays resident on the device, statics: 17-Cheese (%d triangles) + %d boxes" % (n, m, info.triangleCount, boxes))
say("(a) crowd only: the scene with an empty static list against sge_blas_intersect_device(any_instance = 1)")
ms = alternate("blas_intersect_device", "scene_intersect_device")
ref, sc = report("blas_intersect_device", ms["blas_intersect_device"]), report("scene_intersect_device", ms["scene_intersect_device"])
inside = ref.min() <= np.median(sc) <= ref.max()
say("  scene median / reference median = %.3f; %s the spread of the reference's five runs (%.3f .. %.3f ms)" % (
    np.median(sc) / np.median(ref), "inside" if inside else "OUTSIDE", ref.min(), ref.max()))
eng.scene_instances(mesh_of, S.reshape(-1, 16))
say("(b) whole-scene closest hit and (c) occlusion, the same rays")
ms = alternate("scene_intersect_device", "scene_occluded_device")
hitms, occms = report("scene_intersect_device", ms["scene_intersect_device"]), report("scene_occluded_device", ms["scene_occluded_device"])
eng.synchronize()
h = d_h.cpu().numpy().view(abi.blas_hit_dtype)
occ = d_o.cpu().numpy()
say("  %.0f %% of the rays hit (%.0f %% of the hits are static instances); occluded == hit for %d of %d rays" % (
    100 * h["hit"].mean(), 100 * (h["instance"][h["hit"] == 1] >= abi.SCENE_STATIC_BASE).mean(), (occ == h["hit"]).sum(), m))
say("  occlusion median / closest-hit median = %.3f (%s)" % (np.median(occms) / np.median(hitms),
                                                               "not slower" if np.median(occms) <= np.median(hitms) else "SLOWER: a defect"))
eng.close()

if "--variants" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from variant_crowd import settled_crowd
    uniform = {"scene_intersect_device": np.median(hitms), "scene_occluded_device": np.median(occms)}
    ext = float((hi - lo)[[0, 2]].max())
    for mode, what in (("control", "three variants that all hold the full mesh"), ("lod", "full / half / quarter vertex count")):
        # the eye of tools/render_bench.py's camera: above the middle of the crowd's front edge
        eng, P2, per, verts = settled_crowd(sge, n, mode, lambda a, b: (a + b) / 2 + (0.0, 0.18 * ext, 0.62 * ext))
        upload_mesh(eng, 0, cpos, cheese["indices"])
        upload_mesh(eng, 1, bp, bi)
        eng.scene_instances(mesh_of, S.reshape(-1, 16))
        stream = torch.cuda.ExternalStream(eng.stream_handle(), device="cuda:0")
        forms = forms_of(eng)
        say("(%s) mesh variants, %s: vertices per variant %s, characters per variant %s (sge_lod_select); max |position - uniform run's| = %.3g" % (
            mode, what, verts, per, float(np.abs(P2 - P).max())))
        ms = alternate("scene_intersect_device", "scene_occluded_device")
        for k in ("scene_intersect_device", "scene_occluded_device"):
            v = report(k, ms[k])
            say("    median / the uniform line's median = %.3f" % (np.median(v) / uniform[k]))
        eng.synchronize()
        h = d_h.cpu().numpy().view(abi.blas_hit_dtype)
        occ = d_o.cpu().numpy()
        say("  %.0f %% of the rays hit (%.0f %% of the hits are static instances); occluded == hit for %d of %d rays" % (
            100 * h["hit"].mean(), 100 * (h["instance"][h["hit"] == 1] >= abi.SCENE_STATIC_BASE).mean(), (occ == h["hit"]).sum(), m))
        eng.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
