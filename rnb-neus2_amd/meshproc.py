"""Minimal triangle-mesh utilities for the pipeline's last stage and for albedo scaling: OBJ read/write (the layout
save_mesh emits, src/marching_cubes.cu:922-981), connected components, consistent outward orientation — the trimesh
calls of rnb_neus2/pipeline.py:178-219 and albedo_scaling.py:262-263 without trimesh."""
import numpy as np
from scipy import sparse
from scipy.sparse import csgraph


class Mesh:
    def __init__(self, vertices, faces, colors=None):
        self.vertices = np.asarray(vertices, np.float64).reshape(-1, 3)
        self.faces = np.asarray(faces, np.int64).reshape(-1, 3)
        self.colors = None if colors is None else np.asarray(colors, np.float64).reshape(-1, 3)

    @property
    def area(self):
        v = self.vertices[self.faces]
        return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1).sum()

    @property
    def signed_volume(self):
        v = self.vertices[self.faces]
        return np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0

    def vertex_normals(self):
        v = self.vertices[self.faces]
        fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        n = np.zeros_like(self.vertices)
        for k in range(3):
            np.add.at(n, self.faces[:, k], fn)
        l = np.linalg.norm(n, axis=1, keepdims=True)
        return n / np.where(l > 0, l, 1.0)

    def split(self):
        """Connected components (faces sharing a vertex), each with its own compact vertex array."""
        nf = len(self.faces)
        if nf == 0:
            return []
        nv = len(self.vertices)
        g = sparse.coo_matrix((np.ones(3 * nf), (np.repeat(np.arange(nf), 3), self.faces.ravel())), shape=(nf, nv)).tocsr()
        n_comp, labels = csgraph.connected_components(sparse.bmat([[None, g], [g.T, None]]), directed=False)
        labels = labels[:nf]
        out = []
        for c in np.unique(labels):
            f = self.faces[labels == c]
            used, inv = np.unique(f, return_inverse=True)
            out.append(Mesh(self.vertices[used], inv.reshape(-1, 3), None if self.colors is None else self.colors[used]))
        return out

    def fix_normals(self):
        """Make the winding consistent across shared edges (breadth-first per component), then flip components whose
        signed volume is negative so that normals point outward."""
        f = self.faces
        nf = len(f)
        if nf == 0:
            return
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])  # directed edges; edge k of face i is row i + k*nf
        owner = np.tile(np.arange(nf), 3)
        key = np.sort(e, axis=1)
        order = np.lexsort((key[:, 1], key[:, 0]))
        ks = key[order]
        same = np.all(ks[1:] == ks[:-1], axis=1)
        a, b = order[:-1][same], order[1:][same]  # pairs of half-edges on the same undirected edge
        flip_needed = e[a, 0] == e[b, 0]  # same direction in both faces => inconsistent winding
        fa, fb = owner[a], owner[b]
        adj = sparse.coo_matrix((np.ones(len(fa)), (fa, fb)), shape=(nf, nf)).tocsr()
        adj = adj + adj.T
        n_comp, labels = csgraph.connected_components(adj, directed=False)
        # parity propagation: x_b = x_a xor flip_needed along a spanning forest
        parity = {}
        for x, y, w in zip(fa, fb, flip_needed):
            parity[(x, y)] = w
            parity[(y, x)] = w
        flip = np.zeros(nf, bool)
        seen = np.zeros(nf, bool)
        indptr, indices = adj.indptr, adj.indices
        for seed in range(nf):
            if seen[seed]:
                continue
            seen[seed] = True
            queue = [seed]
            while queue:
                cur = queue.pop()
                for nb in indices[indptr[cur]:indptr[cur + 1]]:
                    if not seen[nb]:
                        seen[nb] = True
                        flip[nb] = flip[cur] ^ bool(parity[(cur, nb)])
                        queue.append(nb)
        self.faces = np.where(flip[:, None], f[:, ::-1], f)
        for c in range(n_comp):
            sel = labels == c
            v = self.vertices[self.faces[sel]]
            if np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() < 0:
                self.faces[sel] = self.faces[sel][:, ::-1]


def load_obj(path):
    """`v x y z [r g b]` and `f a[/b[/c]] ...` records (polygons are fan-triangulated); other records are ignored."""
    verts, cols, faces = [], [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                t = line.split()
                verts.append([float(t[1]), float(t[2]), float(t[3])])
                if len(t) >= 7:
                    cols.append([float(t[4]), float(t[5]), float(t[6])])
            elif line.startswith("f "):
                idx = [int(t.split("/")[0]) for t in line.split()[1:]]
                idx = [i - 1 if i > 0 else len(verts) + i for i in idx]
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    return Mesh(verts, faces, cols if len(cols) == len(verts) and cols else None)


def save_obj(path, mesh):
    n = mesh.vertex_normals()
    with open(path, "w") as f:
        if mesh.colors is not None:
            for v, c in zip(mesh.vertices, mesh.colors):
                f.write("v %.8f %.8f %.8f %.6f %.6f %.6f\n" % (v[0], v[1], v[2], c[0], c[1], c[2]))
        else:
            for v in mesh.vertices:
                f.write("v %.8f %.8f %.8f\n" % (v[0], v[1], v[2]))
        for q in n:
            f.write("vn %.8f %.8f %.8f\n" % (q[0], q[1], q[2]))
        for a, b, c in mesh.faces + 1:
            f.write("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c))


def texture_albedo_u8(albedo):
    """The albedo PNG's samples: uint8 RGB, floor(255 * clip(c, 0, 1) + 0.5) of channels 0-2, the values as they are (no colour-space transform), like the vertex colours."""
    c = np.clip(np.asarray(albedo, np.float32)[..., :3].astype(np.float64), 0.0, 1.0)
    return np.floor(255.0 * c + 0.5).astype(np.uint8)


def texture_normal_u16(normal):
    """The normal PNG's samples: uint16 RGB, floor(65535 * clip(n * 0.5 + 0.5, 0, 1) + 0.5) of channels 0-2: an object-space normal map (a texel without a triangle is mid-grey)."""
    c = np.clip(np.asarray(normal, np.float32)[..., :3].astype(np.float64) * 0.5 + 0.5, 0.0, 1.0)
    return np.floor(65535.0 * c + 0.5).astype(np.uint16)


def save_obj_textured(path, mesh, uv, maps):
    """A mesh with the atlas of Context.bake_texture: `path` = X.obj gets `vt` records (three per triangle, in the order of `uv` float32[nt, 3, 2]) and `f a/t/n` faces
    whose corner `corner` of triangle t names vt 3 t + corner + 1; X.mtl names the images; X_albedo.png (8-bit RGB, texture_albedo_u8) and X_normal.png (16-bit RGB,
    texture_normal_u16) are written for the maps of those names in `maps` (name -> float32[S, S, 4], row 0 = the top row); other entries are ignored. The PNGs go through hostlib.png_write."""
    import os
    from . import hostlib

    uv = np.asarray(uv, np.float32).reshape(-1, 3, 2)
    if len(uv) != len(mesh.faces):
        raise ValueError("uv must have one row of three corners per triangle")
    stem = os.path.splitext(str(path))[0]
    base = os.path.basename(stem)
    images = {}
    if maps.get("albedo") is not None:
        images["albedo"] = base + "_albedo.png"
        hostlib.png_write(stem + "_albedo.png", texture_albedo_u8(maps["albedo"]))
    if maps.get("normal") is not None:
        images["normal"] = base + "_normal.png"
        hostlib.png_write(stem + "_normal.png", texture_normal_u16(maps["normal"]))
    with open(stem + ".mtl", "w") as f:
        f.write("newmtl baked\nKa 1.000 1.000 1.000\nKd 1.000 1.000 1.000\nKs 0.000 0.000 0.000\nillum 1\n")
        if "albedo" in images:
            f.write("map_Kd %s\n" % images["albedo"])
        if "normal" in images:
            f.write("norm %s\n" % images["normal"])
    n = mesh.vertex_normals()
    with open(path, "w") as f:
        f.write("mtllib %s.mtl\n" % base)
        for v in mesh.vertices:
            f.write("v %.8f %.8f %.8f\n" % (v[0], v[1], v[2]))
        for q in uv.reshape(-1, 2):
            f.write("vt %.9g %.9g\n" % (q[0], q[1]))
        for q in n:
            f.write("vn %.8f %.8f %.8f\n" % (q[0], q[1], q[2]))
        f.write("usemtl baked\n")
        for t, (a, b, c) in enumerate(mesh.faces + 1):
            f.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a, 3 * t + 1, a, b, 3 * t + 2, b, c, 3 * t + 3, c))
