"""TEST INFRASTRUCTURE: the crowd half of tests/scene_ref.py for a crowd with mesh variants (include/sge_amd_variant_scene.h).

VariantCrowdRef looks like the oracle engine SceneRef(crowd=...) and RenderRef take (`.count`, `.blas_intersect`), and holds one
oracle engine per variant, built like scene_ref._mesh_oracle: the variant's mesh rigidly bound, one oracle character per character
of the crowd that the refit's record assigns to that variant, fed those characters' slices of the GPU's ragged streams and their
instance matrices. A character whose record is `no_variant` (0xFF) is in no engine: a ray that names it misses, no ray reports it.
Hit instances are mapped back to character indices; the parts are composed by scene_ref.compose."""
import numpy as np

import oracle_binding as ob
from scene_ref import _mesh_oracle, compose


class VariantCrowdRef:
    def __init__(self, sge, meshes, records, offsets, positions, normals, tangents, matrices, no_variant=0xFF):
        """meshes: one dict per variant ("positions", "normals", "tangents", "indices", optional "uvs"); records [N] uint8 as the
        refit left them; offsets [N + 1]; positions / normals [total][3] and tangents [total][4]: the ragged streams; matrices
        [N][16] column-major."""
        self.count = len(records)
        self.parts = []
        records = np.asarray(records)
        matrices = np.asarray(matrices, np.float32).reshape(-1, 16)
        for v, mesh in enumerate(meshes):
            sel = np.flatnonzero(records == v)
            if not len(sel):
                continue
            V = len(np.asarray(mesh["positions"]).reshape(-1, 3))
            rows = np.concatenate([np.arange(offsets[c], offsets[c] + V) for c in sel])
            eng = _mesh_oracle(sge, mesh, len(sel))
            ob.skinned_upload(eng, np.ascontiguousarray(positions[rows]), np.ascontiguousarray(normals[rows]), np.ascontiguousarray(tangents[rows]))
            eng.blas_instances(np.ascontiguousarray(matrices[sel]))
            self.parts.append((eng, sel))
        assert all(r == no_variant or r < len(meshes) for r in records.tolist())

    def close(self):
        for eng, _ in self.parts:
            eng.close()

    def blas_intersect(self, origins, directions, instances, min_distance=0.001, max_distance=1e6):
        n = len(np.asarray(origins).reshape(-1, 3))
        ids = np.broadcast_to(np.asarray(instances, np.int64), (n,)).copy()
        answers = []
        for eng, sel in self.parts:
            k = len(sel)
            where = np.searchsorted(sel, ids)
            named = (ids >= 0) & (where < k) & (sel[np.minimum(where, k - 1)] == ids)
            local = np.where(ids < 0, -1, np.where(named, where, k)).astype(np.int32)  # k: names nobody here -> miss
            h = eng.blas_intersect(origins, directions, local, min_distance=min_distance, max_distance=max_distance)
            hit = h["hit"] == 1
            h["instance"][hit] = sel[h["instance"][hit]]
            answers.append(h)
        if not answers:
            raise AssertionError("VariantCrowdRef: no character has a record")
        return compose(answers)
