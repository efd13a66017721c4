"""Triangle-mesh container with the Open3D calls ``gs2mesh_utils/tsdf_utils.py:108-142`` makes (``scale``,
``compute_vertex_normals``, ``cluster_connected_triangles``, ``remove_triangles_by_mask``, ``remove_unreferenced_vertices``,
``o3d.io.write_triangle_mesh``).  Extraction, vertex welding (``gs2m_tsdf_extract_mesh``) and the connected components
(``gs2m_mesh_cluster``) run on the GPU; what is left here is the container, O(n) numpy bookkeeping on the final arrays
(scale, normals, mask / compaction) and the PLY writer.  ``from_triangle_soup`` is the host statement of the weld that the
device path is tested against."""
from __future__ import annotations

import numpy as np


class TriangleMesh:
    def __init__(self, vertices=None, triangles=None, vertex_colors=None):
        self.vertices = np.zeros((0, 3), np.float64) if vertices is None else np.asarray(vertices, np.float64)
        self.triangles = np.zeros((0, 3), np.int32) if triangles is None else np.asarray(triangles, np.int32)
        self.vertex_colors = (np.zeros((0, 3), np.float64) if vertex_colors is None
                              else np.asarray(vertex_colors, np.float64))
        self.vertex_normals = np.zeros((0, 3), np.float64)
        self.triangle_normals = np.zeros((0, 3), np.float64)
        self.edge_index = np.zeros((0, 4), np.int32)   # per vertex, after extraction: the cut edge (Open3D's vertex key)

    # ---- construction from the un-welded GPU output ------------------------------------------
    @staticmethod
    def from_triangle_soup(verts, cols=None, edge_index=None):
        """verts [n,3,3] float64.  With ``edge_index`` [n,3,4] int32 (the cut edge of every emitted vertex: global voxel
        index of its lower corner + axis) the vertices are welded by that key, which is Open3D's own vertex identity
        (ExtractTriangleMesh's edge -> vertex map); without it by position (vertices shared by neighbouring triangles are
        bit-identical) -- the same mesh unless a tsdf value is exactly 0, where up to three edges share one position."""
        v = np.ascontiguousarray(verts, np.float64).reshape(-1, 3)
        if v.shape[0] == 0:
            return TriangleMesh()
        if edge_index is not None:
            key = np.ascontiguousarray(edge_index, np.int32).reshape(-1, 4).view([("", np.int32)] * 4).reshape(-1)
        else:
            key = v.view([("", np.float64)] * 3).reshape(-1)
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        # keep first-appearance order (deterministic, independent of float ordering)
        order = np.argsort(first, kind="stable")
        rank = np.empty_like(order)
        rank[order] = np.arange(order.size)
        tri = rank[inv].reshape(-1, 3).astype(np.int32)
        sel = first[order]
        m = TriangleMesh(v[sel], tri, None if cols is None else np.asarray(cols, np.float64).reshape(-1, 3)[sel])
        if edge_index is not None:
            m.edge_index = np.ascontiguousarray(edge_index, np.int32).reshape(-1, 4)[sel]   # [n_vertices, 4]: Open3D's vertex keys
        return m

    # ---- Open3D API subset -----------------------------------------------------------------
    def scale(self, s, center=(0, 0, 0)):
        c = np.asarray(center, np.float64)
        self.vertices = (self.vertices - c) * float(s) + c
        return self

    def transform(self, transformation):
        """Open3D's ``transform``: v <- (T [v, 1])[:3] / (T [v, 1])[3] in f64; normals, where present, go through the upper
        3 x 3 block as Open3D's do (not renormalised)."""
        T = np.asarray(transformation, np.float64).reshape(4, 4)
        h = self.vertices @ T[:3, :3].T + T[:3, 3]
        w = self.vertices @ T[3, :3] + T[3, 3]
        self.vertices = h / w[:, None]
        for name in ("vertex_normals", "triangle_normals"):
            n = getattr(self, name)
            if n.shape[0]:
                setattr(self, name, n @ T[:3, :3].T)
        return self

    def compute_triangle_normals(self):
        v = self.vertices
        t = self.triangles
        n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
        ln = np.linalg.norm(n, axis=1, keepdims=True)
        self.triangle_normals = n / np.where(ln > 0, ln, 1.0)
        return self

    def compute_vertex_normals(self, on_device=False, lib=None, device=None):
        """Open3D ComputeVertexNormals: sum of the (normalised) normals of the adjacent triangles, normalised.  ``on_device``:
        the same arithmetic on the GPU (``gs2m_mesh_vertex_normals``, bit-identical to the numpy statement below), on the
        triangle indices the extraction left on the device when this mesh still is that mesh, else on an upload of
        ``triangles``."""
        if on_device:
            return self._vertex_normals_device(lib, device)
        self.compute_triangle_normals()
        vn = np.zeros_like(self.vertices)
        for k in range(3):
            np.add.at(vn, self.triangles[:, k], self.triangle_normals)
        ln = np.linalg.norm(vn, axis=1, keepdims=True)
        self.vertex_normals = vn / np.where(ln > 0, ln, 1.0)
        return self

    def _vertex_normals_device(self, lib, device):
        import ctypes as C
        from . import _lib
        import torch
        nv, nt = int(self.vertices.shape[0]), int(self.triangles.shape[0])
        dev = getattr(self, "_dev", None)
        if dev is not None and dev[3] is self.triangles and lib in (None, dev[1]):
            tri_dev, lib, device = dev[0], dev[1], dev[2]
        else:
            lib = lib if lib is not None else _lib.get()
            if device is None:
                device = torch.cuda.current_device() if torch.cuda.is_available() else 0
            tri_dev = _lib.MEMORY.upload(np.ascontiguousarray(self.triangles, np.int32), torch.int32, device) if nt else None
        # handed over as a tensor: every memory policy uploads an f64 tensor as it is
        v_dev = _lib.MEMORY.upload(torch.from_numpy(np.ascontiguousarray(self.vertices, np.float64)), torch.float64, device) if nv else None
        tn_dev = _lib.MEMORY.zeros((nt, 3), np.float64, device)
        vn_dev = _lib.MEMORY.zeros((nv, 3), np.float64, device)
        _lib.check(lib.gs2m_mesh_vertex_normals(int(device), _lib.MEMORY.current_stream(device), nv, _lib.MEMORY.ptr(v_dev), nt,
                                                _lib.MEMORY.ptr(tri_dev), _lib.MEMORY.ptr(tn_dev), _lib.MEMORY.ptr(vn_dev)), lib)
        self.triangle_normals = np.asarray(_lib.MEMORY.download(tn_dev), np.float64).reshape(nt, 3)
        self.vertex_normals = np.asarray(_lib.MEMORY.download(vn_dev), np.float64).reshape(nv, 3)
        return self

    # ---- device attachment -------------------------------------------------------------------
    def attach_device_triangles(self, tri_dev, lib, device):
        """Keep the device copy of ``triangles`` the extraction left behind (valid while ``self.triangles`` is that array)."""
        self._dev = (tri_dev, lib, int(device), self.triangles)

    def __deepcopy__(self, memo):
        import copy
        m = TriangleMesh(self.vertices.copy(), self.triangles.copy(), self.vertex_colors.copy())
        m.vertex_normals, m.triangle_normals, m.edge_index = (copy.deepcopy(self.vertex_normals, memo),
                                                              copy.deepcopy(self.triangle_normals, memo), self.edge_index.copy())
        return m                                   # the device attachment belongs to the original

    def cluster_connected_triangles(self, lib=None, device=None):
        """-> (triangle_clusters[n_tri], cluster_n_triangles[n_clusters], cluster_area[n_clusters]); triangles are connected
        when they share an edge (Open3D ClusterConnectedTriangles; clusters numbered by their first triangle).  The components
        are found on the GPU (``gs2m_mesh_cluster``: union-find over an edge hash table) -- on the triangle indices the
        extraction left on the device when this mesh still is that mesh, else on an upload of ``triangles`` (12 B each);
        the areas are one numpy bincount over the labels."""
        import ctypes as C
        from . import _lib
        n = int(self.triangles.shape[0])
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.float64)
        dev = getattr(self, "_dev", None)
        if dev is not None and dev[3] is self.triangles and lib in (None, dev[1]):
            tri_dev, lib, device = dev[0], dev[1], dev[2]
        else:
            lib = lib if lib is not None else _lib.get()
            import torch
            if device is None:      # the caller's current device, not device 0 (a rank whose GPU is not 0)
                device = torch.cuda.current_device() if torch.cuda.is_available() else 0
            tri_dev = _lib.MEMORY.upload(np.ascontiguousarray(self.triangles, np.int32), torch.int32, device)
        labels_dev = _lib.MEMORY.zeros((n,), np.int32, device)
        count_dev = _lib.MEMORY.zeros((n,), np.int64, device)
        nc = C.c_int64(0)
        # torch's current stream: the zero fills above were queued on it (the NULL stream is not ordered against a
        # non-blocking stream)
        _lib.check(lib.gs2m_mesh_cluster(int(device), _lib.MEMORY.current_stream(device), n, _lib.MEMORY.ptr(tri_dev),
                                         _lib.MEMORY.ptr(labels_dev), _lib.MEMORY.ptr(count_dev), C.byref(nc)), lib)
        labels = np.asarray(_lib.MEMORY.download(labels_dev), np.int32)
        counts = np.asarray(_lib.MEMORY.download(count_dev), np.int64)[: int(nc.value)].copy()
        # triangle areas: component-wise cross product (np.cross / np.linalg.norm on 0.9 M rows were 60 of the 70 ms this call took
        # on C2 -- bench `cluster_ms` -- next to 0.9 ms of kernels)
        v, t = self.vertices, self.triangles
        p0 = v[t[:, 0]]
        a, b = v[t[:, 1]] - p0, v[t[:, 2]] - p0
        cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        area = 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)
        return labels, counts, np.bincount(labels, weights=area, minlength=int(nc.value))

    def remove_triangles_by_mask(self, mask):
        keep = ~np.asarray(mask, bool)
        self.triangles = self.triangles[keep]
        if self.triangle_normals.shape[0] == keep.shape[0]:
            self.triangle_normals = self.triangle_normals[keep]
        return self

    def remove_vertices_by_mask(self, mask):
        """Open3D's ``remove_vertices_by_mask`` (trimesh: ``update_vertices(~mask)`` + ``update_faces``): drop the vertices
        where ``mask`` is True.  The others keep their order -- also those that no triangle uses any more --, a triangle stays
        iff all three of its vertices stay, renumbered, and colours and normals follow the vertices."""
        remove = np.asarray(mask, bool).reshape(-1)
        if remove.shape[0] != self.vertices.shape[0]:
            raise ValueError(f"remove_vertices_by_mask: mask of {remove.shape[0]} for {self.vertices.shape[0]} vertices")
        keep = ~remove
        remap = np.cumsum(keep) - 1
        tri_keep = keep[self.triangles].all(axis=1) if self.triangles.shape[0] else np.zeros(0, bool)
        if self.triangle_normals.shape[0] == tri_keep.shape[0]:
            self.triangle_normals = self.triangle_normals[tri_keep]
        self.triangles = remap[self.triangles[tri_keep]].astype(np.int32).reshape(-1, 3)
        if self.vertex_colors.shape[0] == keep.shape[0]:
            self.vertex_colors = self.vertex_colors[keep]
        if self.vertex_normals.shape[0] == keep.shape[0]:
            self.vertex_normals = self.vertex_normals[keep]
        if self.edge_index.shape[0] == keep.shape[0]:
            self.edge_index = self.edge_index[keep]
        self.vertices = self.vertices[keep]
        return self

    def remove_unreferenced_vertices(self):
        used = np.zeros(self.vertices.shape[0], bool)
        used[self.triangles.reshape(-1)] = True
        remap = np.cumsum(used) - 1
        self.triangles = remap[self.triangles].astype(np.int32)
        self.vertices = self.vertices[used]
        if self.vertex_colors.shape[0] == used.shape[0]:
            self.vertex_colors = self.vertex_colors[used]
        if self.vertex_normals.shape[0] == used.shape[0]:
            self.vertex_normals = self.vertex_normals[used]
        if self.edge_index.shape[0] == used.shape[0]:
            self.edge_index = self.edge_index[used]
        return self

    def has_vertex_normals(self):
        return self.vertex_normals.shape[0] == self.vertices.shape[0] and self.vertices.shape[0] > 0

    def has_vertex_colors(self):
        return self.vertex_colors.shape[0] == self.vertices.shape[0] and self.vertices.shape[0] > 0


def write_triangle_mesh(path, mesh: TriangleMesh):
    """Binary little-endian PLY in the layout ``o3d.io.write_triangle_mesh`` produces for a TriangleMesh:
    double x y z [double nx ny nz] [uchar red green blue], faces as ``list uchar uint vertex_indices``."""
    nv, nt = mesh.vertices.shape[0], mesh.triangles.shape[0]
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    hdr = ["ply", "format binary_little_endian 1.0", "comment Created by gs2mesh_amd", f"element vertex {nv}",
           "property double x", "property double y", "property double z"]
    if mesh.has_vertex_normals():
        fields += [("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8")]
        hdr += ["property double nx", "property double ny", "property double nz"]
    if mesh.has_vertex_colors():
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        hdr += ["property uchar red", "property uchar green", "property uchar blue"]
    hdr += [f"element face {nt}", "property list uchar uint vertex_indices", "end_header"]
    v = np.zeros(nv, dtype=fields)
    v["x"], v["y"], v["z"] = mesh.vertices[:, 0], mesh.vertices[:, 1], mesh.vertices[:, 2]
    if mesh.has_vertex_normals():
        v["nx"], v["ny"], v["nz"] = mesh.vertex_normals[:, 0], mesh.vertex_normals[:, 1], mesh.vertex_normals[:, 2]
    if mesh.has_vertex_colors():
        c = np.clip(np.floor(mesh.vertex_colors * 255.0), 0, 255).astype(np.uint8)   # Open3D: (uint8_t)(c*255) clamped
        v["red"], v["green"], v["blue"] = c[:, 0], c[:, 1], c[:, 2]
    f = np.zeros(nt, dtype=[("n", "u1"), ("i", "<u4", (3,))])
    f["n"] = 3
    f["i"] = mesh.triangles
    with open(path, "wb") as fh:
        fh.write(("\n".join(hdr) + "\n").encode())
        fh.write(v.tobytes())
        fh.write(f.tobytes())
    return True


def read_triangle_mesh(path) -> TriangleMesh:
    """Reader for the files ``write_triangle_mesh`` writes (used by the tests)."""
    with open(path, "rb") as fh:
        assert fh.readline().strip() == b"ply"
        props, nv, nt, cur = [], 0, 0, None
        while True:
            tok = fh.readline().strip().split()
            if tok[0] == b"element":
                cur = tok[1]
                if cur == b"vertex":
                    nv = int(tok[2])
                else:
                    nt = int(tok[2])
            elif tok[0] == b"property" and cur == b"vertex":
                props.append((tok[2].decode(), {"double": "<f8", "float": "<f4", "uchar": "u1"}[tok[1].decode()]))
            elif tok[0] == b"end_header":
                break
        v = np.frombuffer(fh.read(nv * np.dtype(props).itemsize), dtype=props, count=nv)
        f = np.frombuffer(fh.read(nt * 13), dtype=[("n", "u1"), ("i", "<u4", (3,))], count=nt)
    m = TriangleMesh(np.stack([v["x"], v["y"], v["z"]], 1), f["i"].astype(np.int32))
    names = [p[0] for p in props]
    if "nx" in names:
        m.vertex_normals = np.stack([v["nx"], v["ny"], v["nz"]], 1)
    if "red" in names:
        m.vertex_colors = np.stack([v["red"], v["green"], v["blue"]], 1) / 255.0
    return m


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_point_cloud(path) -> np.ndarray:
    """The vertex positions of any PLY whose vertex element comes first -> [N,3] f64: ``binary_little_endian`` or ``ascii``,
    ``x y z`` as float or double among any other scalar vertex properties; later elements (faces) are ignored.  For
    ground-truth point sets and for meshes other programs wrote; ``read_triangle_mesh`` reads this package's own files."""
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, props, nv, cur, first = None, [], 0, None, None
        while True:
            line = fh.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            tok = line.decode("ascii", errors="replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                cur = tok[1]
                first = first or cur
                if cur == "vertex":
                    nv = int(tok[2])
            elif tok[0] == "property" and cur == "vertex":
                if tok[1] == "list" or tok[1] not in _PLY_TYPES:
                    raise ValueError(f"{path}: vertex property {' '.join(tok[1:])} is not a scalar")
                props.append((tok[-1], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        names = [p[0] for p in props]
        if first != "vertex" or not all(a in names for a in "xyz"):
            raise ValueError(f"{path}: the first element must be `vertex` with x, y and z")
        if fmt == "binary_little_endian":
            dt = np.dtype([(n, "<" + t) for n, t in props])
            raw = fh.read(nv * dt.itemsize)
            if len(raw) != nv * dt.itemsize:
                raise ValueError(f"{path}: {nv} vertices declared, the file ends before")
            v = np.frombuffer(raw, dtype=dt, count=nv)
            return np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float64)
        if fmt == "ascii":
            rows = np.loadtxt(fh, dtype=np.float64, max_rows=nv, ndmin=2) if nv else np.zeros((0, len(props)))
            if rows.shape != (nv, len(props)):
                raise ValueError(f"{path}: {nv} vertices of {len(props)} properties declared, found {rows.shape}")
            return np.ascontiguousarray(rows[:, [names.index(a) for a in "xyz"]])
        raise ValueError(f"{path}: format {fmt} (binary_little_endian or ascii)")
