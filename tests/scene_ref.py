"""TEST INFRASTRUCTURE: what the ray scene (include/sge_amd_ray_scene.h) must report, composed from the CPU oracle's triangle scan.

The oracle's blas_intersect scans every triangle of an arbitrary "skinned mesh" with the engine's rayTriangle. Per static mesh this
helper builds one oracle engine whose skinned mesh is that mesh (rigidly bound, the pattern of _custom_mesh_engine in
test_gpu_blas.py), with one oracle character per instance of the mesh: the skinned streams are K copies of the mesh's streams
(ob.skinned_upload), the matrices go in through blas_instances. The crowd, when there is one, is an oracle engine the caller has fed
the GPU's skinned streams. The scene's expected record is the composition of those answers by the rule of the header: the minimum
over (distance bits, scene id, primitive id), character c = scene id c, static instance s = SCENE_STATIC_BASE + s. Occlusion is the
`hit` of that record.
"""
import numpy as np

import oracle_binding as ob

STATIC_BASE = 0x40000000


def columns(mats):
    """[S][4][4] row-major numpy matrices -> [S][16] column-major, as the ABI takes them."""
    return np.ascontiguousarray(np.asarray(mats, np.float32).transpose(0, 2, 1)).reshape(-1, 16)


def _mesh_oracle(sge, mesh, k):
    eng = ob.oracle_engine()
    ybot = sge.assets.YBotAssets()
    eng.upload_skeleton(ybot)
    eng.upload_profiles(ybot.profiles)
    pos = np.ascontiguousarray(mesh["positions"], np.float32).reshape(-1, 3)
    V = len(pos)
    eng.upload_skinned_mesh({"positions": pos, "normals": np.ascontiguousarray(mesh["normals"], np.float32),
                             "tangents": np.ascontiguousarray(mesh["tangents"], np.float32), "boneIndices": np.zeros((V, 4), np.uint16),
                             "boneWeights": np.tile(np.array([1, 0, 0, 0], np.float32), (V, 1)),
                             "indices": np.ascontiguousarray(mesh["indices"], np.uint32)})
    eng.resize(k)
    L = sge.assets.default_locomotion(k, ybot)
    L["flags"] = 0
    eng.upload(bodies=sge.assets.default_bodies(k, np.zeros((k, 3))), params=sge.assets.default_controller_params(k),
               controllers=sge.assets.default_controller_state(k), intents=sge.assets.default_intents(k), locomotion=L,
               actions=sge.assets.default_actions(k))
    eng.blas_build(mesh["indices"])
    if mesh.get("uvs") is not None:
        eng.blas_set_uvs(mesh["uvs"])
    ob.skinned_upload(eng, np.tile(pos, (k, 1)), np.tile(np.asarray(mesh["normals"], np.float32).reshape(-1, 3), (k, 1)),
                      np.tile(np.asarray(mesh["tangents"], np.float32).reshape(-1, 4), (k, 1)))
    return eng


def compose(parts):
    """Hit records whose `instance` fields are scene ids -> per ray the minimum over (distance bits, scene id, primitive id)."""
    best = parts[0].copy()
    for h in parts[1:]:
        kb = (best["distance"].view(np.uint32).astype(np.int64), best["instance"].astype(np.int64), best["primitive"].astype(np.int64))
        kh = (h["distance"].view(np.uint32).astype(np.int64), h["instance"].astype(np.int64), h["primitive"].astype(np.int64))
        less = (kh[0] < kb[0]) | ((kh[0] == kb[0]) & ((kh[1] < kb[1]) | ((kh[1] == kb[1]) & (kh[2] < kb[2]))))
        take = (h["hit"] == 1) & ((best["hit"] == 0) | less)
        best[take] = h[take]
    return best


class SceneRef:
    """meshes: {id: {"positions", "normals", "tangents", "indices", optional "uvs"}}; mesh_of [S]; mats [S][4][4] row-major;
    crowd: an oracle engine with blas_build done and the skinned streams to compare against, or None."""

    def __init__(self, sge, meshes, mesh_of, mats, crowd=None):
        self.mesh_of = np.asarray(mesh_of, np.int32).reshape(-1)
        self.crowd = crowd
        self.parts = {}
        for m in sorted(set(self.mesh_of.tolist())):
            sel = np.flatnonzero(self.mesh_of == m)  # ascending: oracle character k is static instance sel[k]
            self.parts[m] = (_mesh_oracle(sge, meshes[m], len(sel)), sel)
        self.set_matrices(mats)

    def set_matrices(self, mats):
        cols = columns(mats)
        for eng, sel in self.parts.values():
            eng.blas_instances(cols[sel])

    def close(self):
        for eng, _ in self.parts.values():
            eng.close()

    def intersect(self, origins, directions, instances=-1, min_distance=0.001, max_distance=1e6):
        n = len(np.asarray(origins).reshape(-1, 3))
        ids = np.broadcast_to(np.asarray(instances, np.int64), (n,)).copy()
        parts = []
        for eng, sel in self.parts.values():
            k = len(sel)
            s = ids - STATIC_BASE
            where = np.searchsorted(sel, s)
            named = (s >= 0) & (where < k) & (sel[np.minimum(where, k - 1)] == s)
            local = np.where(ids < 0, -1, np.where(named, where, k)).astype(np.int32)  # k: names nothing here -> miss
            h = eng.blas_intersect(origins, directions, local, min_distance=min_distance, max_distance=max_distance)
            hit = h["hit"] == 1
            h["instance"][hit] = STATIC_BASE + sel[h["instance"][hit]]
            parts.append(h)
        if self.crowd is not None:
            nchar = self.crowd.count
            local = np.where(ids < 0, -1, np.where(ids < nchar, ids, nchar)).astype(np.int32)
            parts.append(self.crowd.blas_intersect(origins, directions, local, min_distance=min_distance, max_distance=max_distance))
        if not parts:
            out = np.zeros(n, parts_dtype())
            out["primitive"] = -1
            out["instance"] = -1
            return out
        return compose(parts)


def parts_dtype():
    import importlib
    return importlib.import_module("swift-game-engine_amd").abi.blas_hit_dtype


def assert_records_match(got, want, what=""):
    """The bars of test_gpu_blas.py: hit / primitive / instance exact, floats within 1e-6 * max(1, |ref|.max())."""
    for f in ("hit", "primitive", "instance"):
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5].ravel(), got[f][got[f] != want[f]][:5], want[f][got[f] != want[f]][:5])
    for f in ("distance", "bary", "geomNormal", "normal", "tangent", "bitangent", "uv"):
        err = np.abs(got[f] - want[f]).max()
        print("%s %s: max |diff| = %.3g (bar %.3g)" % (what, f, err, 1e-6 * max(1.0, np.abs(want[f]).max())))
        assert err <= 1e-6 * max(1.0, np.abs(want[f]).max()), (what, f, err)
