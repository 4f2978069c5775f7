"""SDF-on-a-grid callers of the fused no-grad kernel and the mesh procedure on top of them (reference:
code/utils/plots.py:110-271).

The reference's mesh extraction evaluates the SDF on resolution^3 points in 10 000-point chunks, each a
9-GEMM eager forward plus a device->host copy (64 M evaluations at resolution 400), then hands the volume to
skimage's marching cubes.  Here the volume is produced by the fused kernel (csrc/hm_sdf.hip, ~32 M points/s on
one MI355X) in a few large launches and comes back in exactly the layout the reference passes to
``measure.marching_cubes`` (axis order, spacing, origin), so the CPU part (marching cubes / trimesh export -
third-party, not part of the hot path) is unchanged.

get_surface_high_res_mesh (plots.py:146-224) runs entirely on this library: the SDF volumes come from the fused kernel
on device-generated lattices, the meshes from ops.marching_cubes (csrc/hm_mesh.hip), and TriMesh stands in for the
part of trimesh.Trimesh the reference's callers use.
"""
import math
import os

import numpy as np
import torch

from .. import ops


def get_grid_uniform(resolution, device=None):
    """plots.py:227-238: the [-1,1]^3 lattice in meshgrid('xy') order; ``grid_points`` [res^3, 3] fp32."""
    x = np.linspace(-1.0, 1.0, resolution)
    y = x
    z = x
    xx, yy, zz = np.meshgrid(x, y, z)
    grid_points = torch.tensor(np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T, dtype=torch.float)
    if device is not None:
        grid_points = grid_points.to(device)
    return {"grid_points": grid_points, "shortest_axis_length": 2.0, "xyz": [x, y, z], "shortest_axis_index": 0}


def _grid_axes(points, resolution, eps=0.2):
    """the axes of get_grid's lattice: (x, y, z, shortest axis length, shortest axis index)"""
    pts = points.detach().cpu()
    input_min = torch.min(pts, dim=0)[0].squeeze().numpy()
    input_max = torch.max(pts, dim=0)[0].squeeze().numpy()
    shortest_axis = int(np.argmin(input_max - input_min))
    lin = np.linspace(input_min[shortest_axis] - eps, input_max[shortest_axis] + eps, resolution)
    length = np.max(lin) - np.min(lin)
    step = length / (lin.shape[0] - 1)
    axes = [None, None, None]
    for a in range(3):
        axes[a] = lin if a == shortest_axis else np.arange(input_min[a] - eps, input_max[a] + step + eps, step)
    return axes[0], axes[1], axes[2], length, shortest_axis


def get_grid(points, resolution, device=None, eps=0.2):
    """plots.py:240-271: lattice around a point cloud, `resolution` samples along its shortest axis."""
    x, y, z, length, shortest_axis = _grid_axes(points, resolution, eps)
    xx, yy, zz = np.meshgrid(x, y, z)
    grid_points = torch.tensor(np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T, dtype=torch.float)
    if device is not None:
        grid_points = grid_points.to(device)
    return {"grid_points": grid_points, "shortest_axis_length": length, "xyz": [x, y, z],
            "shortest_axis_index": shortest_axis}


@torch.no_grad()
def sdf_on_points(sdf, points, chunk=1 << 22):
    """sdf(points) for a long point list; `sdf` is ImplicitNetwork.sdf (fused kernel) or any callable [n,3]->[n]."""
    out = torch.empty(points.shape[0], dtype=torch.float32, device=points.device)
    for i in range(0, points.shape[0], chunk):
        out[i:i + chunk] = sdf(points[i:i + chunk]).reshape(-1)
    return out


def sdf_volume(sdf, grid, chunk=1 << 22):
    """The arguments the reference gives to ``measure.marching_cubes`` (plots.py:122-128): volume [nx, ny, nz]
    (the meshgrid's [ny, nx, nz] transposed), isotropic spacing, and the origin the vertices are shifted by."""
    z = sdf_on_points(sdf, grid["grid_points"], chunk).cpu().numpy().astype(np.float32)
    xs, ys, zs = grid["xyz"]
    volume = z.reshape(ys.shape[0], xs.shape[0], zs.shape[0]).transpose([1, 0, 2])
    d = xs[2] - xs[1]
    return {"volume": volume, "spacing": (d, d, d), "origin": np.array([xs[0], ys[0], zs[0]]),
            "has_surface": not (np.min(z) > 0 or np.max(z) < 0)}


def get_surface_mesh(sdf, resolution=100, device="cuda"):
    """plots.py:110-145 without the plotly / trimesh export: (verts, faces, normals) of the zero level set, or None
    if the volume has no sign change.  Needs scikit-image for marching cubes (as the reference does)."""
    vol = sdf_volume(sdf, get_grid_uniform(resolution, device))
    if not vol["has_surface"]:
        return None
    try:
        from skimage import measure
    except ImportError as err:   # third-party CPU step; the volume above is the GPU part
        raise ImportError("marching cubes needs scikit-image (the reference uses skimage.measure.marching_cubes); "
                          "use sdf_volume() to get the SDF volume without it") from err
    verts, faces, normals, _ = measure.marching_cubes(volume=vol["volume"], level=0, spacing=vol["spacing"])
    return verts + vol["origin"], faces, -normals


# =========================================================================================
# mesh object and the reference's high-resolution mesh procedure
# =========================================================================================
class TriMesh:
    """The part of trimesh.Trimesh the reference's mesh callers use (eval.py: world transform, largest component,
    .ply export; plots.py: .ply export): vertices [V,3] float64, faces [F,3] int64, vertex_normals [V,3] (the given
    ones, else area-weighted face normals), area, apply_transform, split, export.  vertex_colors [V,3] uint8, optional
    (evaluation.color.color_mesh and colors_to_uint8 make them): split gathers them, apply_transform keeps them and
    export writes them after the normals.  texture [Ha,Wa,3] uint8 with face_uvs [F,3,2] (ops.TextureAtlas.image
    through colors_to_uint8, and .face_uvs), optional and given together: split gathers the faces' coordinates,
    export_obj writes them; the .ply export does not carry them."""

    def __init__(self, vertices, faces, vertex_normals=None, vertex_colors=None, texture=None, face_uvs=None):
        self.vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        self._normals = None if vertex_normals is None else np.asarray(vertex_normals, np.float64).reshape(-1, 3)
        self.vertex_colors = None
        if vertex_colors is not None:
            colors = np.asarray(vertex_colors)
            if colors.dtype != np.uint8 or colors.shape != self.vertices.shape:
                raise ValueError("TriMesh: vertex_colors must be uint8 [V, 3] (colors_to_uint8)")
            self.vertex_colors = colors
        self.texture = self.face_uvs = None
        if texture is not None or face_uvs is not None:
            tex = None if texture is None else np.asarray(texture)
            uvs = None if face_uvs is None else np.asarray(face_uvs, np.float64)
            if tex is None or tex.dtype != np.uint8 or tex.ndim != 3 or tex.shape[2] != 3 or 0 in tex.shape:
                raise ValueError("TriMesh: texture must be uint8 [Ha, Wa, 3], given together with face_uvs")
            if uvs is None or uvs.shape != (len(self.faces), 3, 2):
                raise ValueError("TriMesh: face_uvs must be [F, 3, 2], given together with texture")
            self.texture, self.face_uvs = tex, uvs

    def _cross(self):
        v = self.vertices[self.faces]
        return np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])

    @property
    def area_faces(self):
        return 0.5 * np.linalg.norm(self._cross(), axis=1)

    @property
    def area(self):
        return float(self.area_faces.sum())

    @property
    def vertex_normals(self):
        if self._normals is None:
            acc = np.zeros_like(self.vertices)
            cr = self._cross()
            for m in range(3):
                np.add.at(acc, self.faces[:, m], cr)
            nrm = np.linalg.norm(acc, axis=1, keepdims=True)
            self._normals = np.divide(acc, nrm, out=np.zeros_like(acc), where=nrm > 0)
        return self._normals

    @property
    def is_watertight(self):
        """every undirected edge in exactly two faces"""
        e = np.sort(np.concatenate([self.faces[:, [0, 1]], self.faces[:, [1, 2]], self.faces[:, [2, 0]]]), axis=1)
        _, cnt = np.unique(e[:, 0] * (len(self.vertices) + 1) + e[:, 1], return_counts=True)
        return len(self.faces) > 0 and bool(np.all(cnt == 2))

    def apply_transform(self, matrix):
        """x -> M[:3,:3] x + M[:3,3]; normals by the inverse transpose; a reflection reverses the winding"""
        m = np.asarray(matrix, dtype=np.float64)
        if m.shape != (4, 4):
            raise ValueError("TriMesh.apply_transform: a 4x4 matrix expected")
        lin = m[:3, :3]
        normals = None if self._normals is None else self._normals @ np.linalg.inv(lin)
        self.vertices = self.vertices @ lin.T + m[:3, 3]
        if normals is not None:
            nrm = np.linalg.norm(normals, axis=1, keepdims=True)
            self._normals = np.divide(normals, nrm, out=np.zeros_like(normals), where=nrm > 0)
        if np.linalg.det(lin) < 0:
            self.faces = np.ascontiguousarray(self.faces[:, ::-1])
        return self

    def split(self, only_watertight=False):
        """connected components through shared vertices, in the order of their lowest vertex"""
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        f = self.faces
        nv = len(self.vertices)
        if len(f) == 0:
            return []
        rows = np.concatenate([f[:, 0], f[:, 1]])
        cols = np.concatenate([f[:, 1], f[:, 2]])
        graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nv, nv))
        _, label = connected_components(graph, directed=False)
        face_label = label[f[:, 0]]
        out = []
        for lab in np.unique(label[np.unique(f)]):
            ff = f[face_label == lab]
            used, inv = np.unique(ff, return_inverse=True)
            normals = None if self._normals is None else self._normals[used]
            colors = None if self.vertex_colors is None else self.vertex_colors[used]
            uvs = None if self.face_uvs is None else self.face_uvs[face_label == lab]
            part = TriMesh(self.vertices[used], inv.reshape(-1, 3), normals, colors, self.texture, uvs)
            if not only_watertight or part.is_watertight:
                out.append(part)
        return out

    def export(self, file_obj=None, file_type="ply"):
        """binary little-endian PLY: float32 x y z nx ny nz (+ uchar red green blue with vertex_colors), faces as
        (uchar 3, int32 x3); bytes when file_obj is None, else written to the path or binary file object"""
        if file_type != "ply":
            raise ValueError("TriMesh.export: only file_type='ply' is supported")
        names = ["x", "y", "z", "nx", "ny", "nz"]
        rgb = ["red", "green", "blue"] if self.vertex_colors is not None else []
        vdt = np.dtype([(n, "<f4") for n in names] + [(n, "u1") for n in rgb])
        vert = np.empty(len(self.vertices), vdt)
        cols = np.concatenate([self.vertices, self.vertex_normals], axis=1)
        for c, n in enumerate(names):
            vert[n] = cols[:, c]
        for c, n in enumerate(rgb):
            vert[n] = self.vertex_colors[:, c]
        face = np.empty(len(self.faces), np.dtype([("count", "u1"), ("index", "<i4", (3,))]))
        face["count"] = 3
        face["index"] = self.faces
        head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(vert)}"]
        head += [f"property float {n}" for n in names] + [f"property uchar {n}" for n in rgb]
        head += [f"element face {len(face)}", "property list uchar int vertex_indices", "end_header", ""]
        data = "\n".join(head).encode("ascii") + vert.tobytes() + face.tobytes()
        if file_obj is None:
            return data
        if hasattr(file_obj, "write"):
            file_obj.write(data)
        else:
            with open(file_obj, "wb") as fh:
                fh.write(data)
        return None

    def export_obj(self, path):
        """the textured mesh as Wavefront OBJ: `path`.obj (v, vn, vt, f a/t/n with one vt per face corner; %.9g keeps
        every fp32 value), `path`.mtl (one material whose map_Kd is the image) and `path`.png (the texture, row 0 on
        top; vt's v axis points up).  `path` is taken without its .obj suffix.  Returns the three paths."""
        if self.texture is None:
            raise ValueError("TriMesh.export_obj: the mesh has no texture (TriMesh(texture=, face_uvs=))")
        from PIL import Image
        base = path[:-4] if str(path).lower().endswith(".obj") else str(path)
        name = os.path.basename(base)
        Image.fromarray(np.ascontiguousarray(self.texture)).save(base + ".png")
        with open(base + ".mtl", "w") as fh:
            fh.write(f"newmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
        a = self.faces + 1
        t = np.arange(1, 3 * len(a) + 1, dtype=np.int64).reshape(-1, 3)
        lines = [f"mtllib {name}.mtl", f"usemtl {name}"]
        lines += ["v %.9g %.9g %.9g" % tuple(v) for v in self.vertices]
        lines += ["vn %.9g %.9g %.9g" % tuple(v) for v in self.vertex_normals]
        lines += ["vt %.17g %.17g" % tuple(v) for v in self.face_uvs.reshape(-1, 2)]
        lines += ["f " + " ".join(f"{a[i, m]}/{t[i, m]}/{a[i, m]}" for m in range(3)) for i in range(len(a))]
        with open(base + ".obj", "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return base + ".obj", base + ".mtl", base + ".png"


def colors_to_uint8(colors):
    """uint8 [V,3] of colours in the dataset's [-1, 1] range (a tensor or an array): rint(clip((c + 1) / 2, 0, 1) * 255),
    half to even; what TriMesh(vertex_colors=) takes"""
    c = np.asarray(colors.detach().cpu() if isinstance(colors, torch.Tensor) else colors, np.float64)
    return np.rint(np.clip((c + 1.0) / 2.0, 0.0, 1.0) * 255.0).astype(np.uint8).reshape(-1, 3)


@torch.no_grad()
def _lattice_sdf(sdf, axes, device, rot=None, shift=None, chunk=1 << 22):
    """sdf on the meshgrid('xy') lattice of the numpy axes (x, y, z), points generated on the device chunk by chunk
    (no host lattice): a flat [ny*nx*nz] tensor in get_grid's point order.  rot / shift: the points are rotated into
    world space as p @ rot + shift (fp32, the reference's bmm(vecs^T, p) + s_mean)."""
    ax = [torch.as_tensor(np.asarray(a), dtype=torch.float32, device=device) for a in axes]
    nx, ny, nz = (a.numel() for a in ax)
    n = nx * ny * nz
    out = torch.empty(n, dtype=torch.float32, device=device)
    for s in range(0, n, chunk):
        q = torch.arange(s, min(s + chunk, n), dtype=torch.int64, device=device)
        k = q % nz
        i = (q // nz) % nx
        j = q // (nz * nx)
        p = torch.stack([ax[0][i], ax[1][j], ax[2][k]], dim=1)
        if rot is not None:
            p = p @ rot + shift
        out[s:s + chunk] = sdf(p).reshape(-1)
    return out


def _mesh_on_lattice(sdf, axes, device, rot=None, shift=None):
    """marching cubes of sdf's zero set on the lattice (vertices in lattice coordinates from the first point), or None
    without a sign change"""
    x, y, z = axes
    z_flat = _lattice_sdf(sdf, axes, device, rot, shift)
    lo, hi = torch.aminmax(z_flat)
    if lo.item() > 0 or hi.item() < 0:
        return None
    volume = z_flat.view(len(y), len(x), len(z)).permute(1, 0, 2)    # [nx, ny, nz] view, as sdf_volume's transpose
    d = float(x[2] - x[1])
    return ops.marching_cubes(volume, 0.0, (d, d, d))


def lattice_points(axes, q, rot=None, shift=None):
    """The points [n, 3] fp32 (device) with linear indices q (int64, volume order (i*ny + j)*nz + k) of the lattice
    of the axes (x, y, z), taken to p @ rot + shift when given - from the generator of ops.marching_cubes_sparse, so
    sdf(lattice_points(axes, arange(nx*ny*nz))).view(nx, ny, nz) is the volume whose ops.marching_cubes the sparse
    call reproduces."""
    return ops.lattice_points([np.asarray(a) if not torch.is_tensor(a) else a for a in axes], q, rot, shift)


def _surface_moments(mesh):
    """(mean [3], covariance [3,3]) of the uniform distribution on the mesh surface, exact from its triangles"""
    v = mesh.vertices[mesh.faces]
    a = mesh.area_faces
    s = v.sum(axis=1)
    mean = (a[:, None] * s).sum(0) / (3.0 * a.sum())
    second = np.einsum("t,tmi,tmj->ij", a, v, v) + np.einsum("t,ti,tj->ij", a, s, s)
    cov = second / (12.0 * a.sum()) - np.outer(mean, mean)
    return mean, cov


def get_surface_high_res_mesh(sdf, resolution=100, device="cuda", sparse=False, largest_component=False,
                              simplify=None):
    """plots.py:146-224: the zero level set of `sdf` on a lattice aligned with the principal axes of a coarse mesh's
    largest component, `resolution` samples along its shortest axis; a TriMesh in world space, or None without a
    sign change.  Two deliberate deviations (mesh extraction): the principal axes come from the exact
    area-weighted surface moments of the coarse component (the reference: 10 000 random trimesh.sample points), and
    the lattices are generated on the device chunk by chunk (no host lattice).

    sparse=True evaluates the aligned lattice only near the surface (ops.marching_cubes_sparse, seeded with the coarse
    mesh's vertices of all components): the mesh of the full lattice except for components that the coarse 100^3
    lattice does not see, which are absent as a whole.  Its vertices differ from sparse=False in the last bits (the
    lattice points are generated by another fp32 expression).  The lattice may exceed 2^31 points.

    largest_component=True keeps only the fine mesh's component of the largest area (ops.mesh_largest_component) - the
    cleanup evaluation/eval.py applies to every fine mesh, mesh.split(only_watertight=False) and the part at the
    areas' argmax - on the device, so that only that component is downloaded: the TriMesh
    max(get_surface_high_res_mesh(...).split(only_watertight=False), key=area), bit for bit.  The component is taken
    from the world-space fp32 vertices, the ones the host split would see: the transform of all vertices is a [V,3] x
    [3,3] product, and selecting rows afterwards cannot change their bits.

    simplify=k (a positive number; None leaves the mesh as it is) decimates the fine mesh by vertex clustering on a grid
    of k times the fine lattice spacing (ops.mesh_simplify: quadric placement from the SDF normals) on the device, so
    that only the simplified mesh is downloaded.  It is applied to the world-space mesh, after largest_component when
    both are given: the component choice sees the full mesh, as eval.py's does.  Clustering does not preserve
    manifoldness."""
    if simplify is not None and not (isinstance(simplify, (int, float)) and math.isfinite(simplify) and simplify > 0):
        raise ValueError("get_surface_high_res_mesh: simplify must be a positive finite number or None")
    lin = np.linspace(-1.0, 1.0, 100)      # the coarse 100^3 grid of get_grid_uniform(100)
    coarse = _mesh_on_lattice(sdf, (lin, lin, lin), device)
    if coarse is None:
        return None
    verts, faces, normals = (t.cpu().numpy() for t in coarse)
    mesh_low_res = TriMesh(verts + np.array([lin[0], lin[0], lin[0]]), faces, normals)
    components = mesh_low_res.split(only_watertight=False)
    areas = np.array([c.area for c in components], dtype=np.float64)
    mesh_low_res = components[int(areas.argmax())]

    # center and align
    s_mean, s_cov = _surface_moments(mesh_low_res)
    vecs = torch.linalg.eigh(torch.from_numpy(s_cov))[1].transpose(0, 1)
    if torch.det(vecs) < 0:
        vecs = torch.mm(torch.tensor([[1, 0, 0], [0, 0, 1], [0, 1, 0]], dtype=vecs.dtype), vecs)
    helper = (torch.from_numpy(mesh_low_res.vertices) - torch.from_numpy(s_mean)) @ vecs.transpose(0, 1)
    x, y, z, _, _ = _grid_axes(helper, resolution)

    rot = vecs.to(device=device, dtype=torch.float32)
    shift = torch.from_numpy(s_mean).to(device=device, dtype=torch.float32)
    if sparse:
        seeds = (torch.from_numpy(verts + lin[0]) - torch.from_numpy(s_mean)) @ vecs.transpose(0, 1)
        d = float(x[2] - x[1])
        fine = ops.marching_cubes_sparse(sdf, [torch.as_tensor(a, dtype=torch.float32, device=device)
                                               for a in (x, y, z)], (d, d, d), seeds, 0.0, rot, shift)
        if fine[0].shape[0] == 0:
            return None
    else:
        fine = _mesh_on_lattice(sdf, (x, y, z), device, rot, shift)
        if fine is None:
            return None
    verts, faces, normals = fine
    origin = torch.tensor([[x[0], y[0], z[0]]], dtype=torch.float32, device=device) @ rot + shift  # grid_points[0]
    verts = verts @ rot + origin
    normals = normals @ rot
    if largest_component:
        verts, faces, normals = ops.mesh_largest_component(verts.contiguous(), faces.contiguous(),
                                                           normals.contiguous())
    if simplify is not None:
        verts, faces, normals, _ = ops.mesh_simplify(verts.contiguous(), faces.contiguous(), normals.contiguous(),
                                                     cell=simplify * float(x[2] - x[1]))
    return TriMesh(verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy())
