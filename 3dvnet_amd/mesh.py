"""Triangle meshes from TSDF volumes on the device: marching cubes (``csrc/mesh.hip`` behind ``v3d_mesh_count_f32`` /
``v3d_mesh_extract_f32``) with what ``mv3d/eval/tsdf_atlas.py`` does around its marching-cubes call -- ``TSDF.get_mesh``
(:161-253) and the ``tsdf_point_cloud`` attribute of ``get_tsdf`` (:465-481).  This module is the plumbing:

  * ``extract``         volume (+ colour volume) -> vertices, colours, triangles as device tensors;
  * ``TriangleMesh``    a plain holder of those tensors with ``write_ply``;
  * ``read_ply_points`` reads the vertices of a file ``write_ply`` wrote (the reference's ``o3d.io.write_triangle_mesh`` /
                        ``read_point_cloud`` round trip; both run on the host);
  * ``read_triangle_mesh``  reads a binary triangle-mesh PLY of someone else's making (ScanNet's ``*_vh_clean_2.ply``, the
                        file ``scene_info['gt_mesh']`` names; the reference's ``o3d.io.read_triangle_mesh``) on the host.

The triangulation is this project's own rule (``scripts/gen_mc_table.py``), not skimage's Lewiner tables: the vertex SET -- one
vertex per sign-changing grid edge, which is all the 3D metrics read -- is defined by the volume alone, the triangles between
them and the exact vertex positions are not those of skimage.  Where a corner holds exactly 0 several vertices
coincide at that corner and the triangles between them are degenerate.

There is no CPU fallback: without the library or a HIP device ``extract`` raises ``V3DLibraryError``.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MODE_MESH, MODE_POINT_CLOUD = 0, 1          # V3D_MESH_MODE_* of include/v3d.h


def extract(tsdf_vol, color_vol, voxel_size, origin, mode=MODE_MESH):
    """tsdf_vol [nx, ny, nz] fp32 and color_vol [3, nx, ny, nz] fp32 (or None) on a HIP device, origin (3 values) ->
    ``(vertices [V, 3] fp32 world, colours [V, 3] uint8 | None, triangles [F, 3] int32)`` on that device, in the
    deterministic order of include/v3d.h.  ``MODE_MESH``: the reference's ``get_mesh`` rules (bad vertices removed, colours
    in channel order [2, 1, 0], empty-mesh rule); ``MODE_POINT_CLOUD``: every vertex, colours floored in channel order, no
    triangles.  One 8-byte read-back (the two counts) sizes the outputs."""
    lib = _lib.load()
    if not torch.cuda.is_available() or not torch.is_tensor(tsdf_vol) or not tsdf_vol.is_cuda:
        raise _lib.V3DLibraryError('mesh.extract: the volume must live on a HIP device (no CPU fallback)')
    if tsdf_vol.dim() != 3 or tsdf_vol.dtype != torch.float32:
        raise ValueError('mesh.extract: fp32 [nx, ny, nz] expected, got %s %s' % (tsdf_vol.dtype, tuple(tsdf_vol.shape)))
    dev = tsdf_vol.device
    nx, ny, nz = (int(v) for v in tsdf_vol.shape)
    if min(nx, ny, nz) < 1 or nx * ny * nz >= 2 ** 31:
        raise ValueError('mesh.extract: volume %s (positive, fewer than 2^31 voxels)' % ((nx, ny, nz),))
    vol = tsdf_vol.detach().contiguous()
    col = None
    if color_vol is not None:
        if tuple(color_vol.shape) != (3, nx, ny, nz) or color_vol.dtype != torch.float32 or color_vol.device != dev:
            raise ValueError('mesh.extract: the colour volume must be fp32 [3, nx, ny, nz] on the same device')
        col = color_vol.detach().contiguous()
    org = (ctypes.c_float * 3)(*[float(v) for v in torch.as_tensor(origin).detach().reshape(3).cpu()])
    ws = torch.empty(max(int(lib.v3d_mesh_workspace_bytes(nx, ny, nz)), 256), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    stream = _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        _lib.check(lib.v3d_mesh_count_f32(vol.data_ptr(), nx, ny, nz, int(mode), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                          stream), 'v3d_mesh_count_f32')
        n_v, n_f = (int(v) for v in counts.cpu())
        if n_v < 0 or n_f < 0:
            raise _lib.V3DLibraryError('mesh.extract: the mesh has 2^31 or more vertices or triangles')
        verts = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
        colors = None if col is None else torch.empty((n_v, 3), dtype=torch.uint8, device=dev)
        tris = torch.empty((n_f, 3), dtype=torch.int32, device=dev)
        if n_v > 0:
            _lib.check(lib.v3d_mesh_extract_f32(vol.data_ptr(), _lib.ptr(col), nx, ny, nz, float(voxel_size), org, int(mode),
                                                verts.data_ptr(), _lib.ptr(colors), n_v, tris.data_ptr(), n_f, ws.data_ptr(),
                                                ws.numel(), stream), 'v3d_mesh_extract_f32')
    return verts, colors, tris


class TriangleMesh:
    """Plain holder of a mesh's tensors (where they live): ``vertices`` [V, 3] fp32, ``triangles`` [F, 3] int32,
    ``vertex_colors_u8`` [V, 3] uint8 or None (stored channel order, for ``get_mesh`` the reference's [2, 1, 0])."""

    def __init__(self, vertices=None, triangles=None, vertex_colors_u8=None):
        self.vertices = torch.zeros((0, 3), dtype=torch.float32) if vertices is None else vertices
        self.triangles = torch.zeros((0, 3), dtype=torch.int32, device=self.vertices.device) if triangles is None else triangles
        self.vertex_colors_u8 = vertex_colors_u8

    @property
    def vertex_colors(self):
        """[V, 3] fp32 in [0, 1] = bytes / 255 (None without colour)."""
        return None if self.vertex_colors_u8 is None else self.vertex_colors_u8.float() / 255.

    @property
    def points(self):
        """The vertices: what ``metrics3d`` reads from any object with ``.points``."""
        return self.vertices

    def write_ply(self, path):
        """Binary little-endian PLY on the host: double x y z, uchar red green blue (when the mesh has colours), faces as
        uchar count + int indices."""
        v = self.vertices.detach().cpu().numpy().astype('<f8').reshape(-1, 3)
        f = self.triangles.detach().cpu().numpy().astype('<i4').reshape(-1, 3)
        c = None if self.vertex_colors_u8 is None else self.vertex_colors_u8.detach().cpu().numpy().astype(np.uint8).reshape(-1, 3)
        head = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % v.shape[0], 'property double x',
                'property double y', 'property double z']
        fields = [('x', '<f8'), ('y', '<f8'), ('z', '<f8')]
        if c is not None:
            head += ['property uchar red', 'property uchar green', 'property uchar blue']
            fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        head += ['element face %d' % f.shape[0], 'property list uchar int vertex_indices', 'end_header']
        rows = np.empty(v.shape[0], dtype=np.dtype(fields))
        rows['x'], rows['y'], rows['z'] = v[:, 0], v[:, 1], v[:, 2]
        if c is not None:
            rows['red'], rows['green'], rows['blue'] = c[:, 0], c[:, 1], c[:, 2]
        faces = np.empty(f.shape[0], dtype=np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
        faces['n'], faces['i'] = 3, f
        with open(path, 'wb') as out:
            out.write(('\n'.join(head) + '\n').encode('ascii'))
            out.write(rows.tobytes())
            out.write(faces.tobytes())


def read_ply(path):
    """A file ``TriangleMesh.write_ply`` wrote -> ``(vertices [V, 3] float64, colours [V, 3] uint8 | None, triangles [F, 3]
    int32)`` NumPy arrays.  Not a general PLY reader."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    head = data[:end].decode('ascii').split('\n')
    if head[0] != 'ply' or head[1] != 'format binary_little_endian 1.0':
        raise ValueError('read_ply: %s was not written by TriangleMesh.write_ply' % path)
    n_v = n_f = None
    props = []
    for line in head[2:]:
        w = line.split()
        if w[:2] == ['element', 'vertex']:
            n_v = int(w[2])
        elif w[:2] == ['element', 'face']:
            n_f = int(w[2])
        elif w[:1] == ['property'] and n_f is None:
            props.append((w[2], {'double': '<f8', 'uchar': 'u1'}[w[1]]))
    names = [p[0] for p in props]
    if n_v is None or n_f is None or names[:3] != ['x', 'y', 'z'] or names[3:] not in ([], ['red', 'green', 'blue']):
        raise ValueError('read_ply: unexpected header in %s' % path)
    vt = np.dtype(props)
    ft = np.dtype([('n', 'u1'), ('i', '<i4', (3,))])
    if len(data) != end + n_v * vt.itemsize + n_f * ft.itemsize:
        raise ValueError('read_ply: %s is truncated' % path)
    rows = np.frombuffer(data, dtype=vt, count=n_v, offset=end)
    faces = np.frombuffer(data, dtype=ft, count=n_f, offset=end + n_v * vt.itemsize)
    verts = np.stack((rows['x'], rows['y'], rows['z']), axis=1).astype(np.float64)
    cols = np.stack((rows['red'], rows['green'], rows['blue']), axis=1) if len(names) == 6 else None
    return verts, cols, faces['i'].astype(np.int32)


def read_ply_points(path):
    """The vertices of a file ``write_ply`` wrote, [V, 3] float64 (the reference's ``o3d.io.read_point_cloud(path).points``)."""
    return read_ply(path)[0]


_PLY_SCALARS = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': '<i2', 'int16': '<i2', 'ushort': '<u2',
                'uint16': '<u2', 'int': '<i4', 'int32': '<i4', 'uint': '<u4', 'uint32': '<u4', 'float': '<f4', 'float32': '<f4',
                'double': '<f8', 'float64': '<f8'}


def read_triangle_mesh(path):
    """A binary little-endian PLY triangle mesh -> ``TriangleMesh`` on the host (vertices fp32, triangles int32, colours uint8
    or None).  Accepted: a ``vertex`` element with ``float`` or ``double`` ``x y z`` and any further scalar properties (skipped,
    except ``red green blue`` as ``uchar``, which are kept), followed by a ``face`` element whose only property is a list of
    ``uchar`` count and ``int`` / ``uint`` indices, every face a triangle -- the layout of ScanNet's ``*_vh_clean_2.ply`` and
    of ``write_ply``.  Anything else raises ``ValueError`` with the reason."""
    with open(path, 'rb') as f:
        data = f.read()

    def bad(why):
        return ValueError('read_triangle_mesh: %s: %s' % (path, why))

    mark = data.find(b'end_header')
    if not data.startswith(b'ply') or mark < 0:
        raise bad('not a PLY file (no "ply" ... "end_header")')
    end = data.find(b'\n', mark)
    if end < 0:
        raise bad('the header does not end with a newline')
    end += 1
    try:
        lines = [ln.strip() for ln in data[:mark].decode('ascii').splitlines()]
    except UnicodeDecodeError:
        raise bad('the header is not ASCII')
    lines = [ln for ln in lines[1:] if ln and not ln.startswith(('comment', 'obj_info'))]
    if not lines or lines[0].split() != ['format', 'binary_little_endian', '1.0']:
        raise bad('only "format binary_little_endian 1.0" is read, the file says %r' % (lines[0] if lines else ''))
    elements = []                                   # [name, count, [property words]]
    for ln in lines[1:]:
        w = ln.split()
        if w[0] == 'element' and len(w) == 3 and w[2].isdigit():
            elements.append([w[1], int(w[2]), []])
        elif w[0] == 'property' and elements and len(w) >= 3:
            elements[-1][2].append(w[1:])
        else:
            raise bad('header line %r' % ln)
    if [e[0] for e in elements[:2]] != ['vertex', 'face']:
        raise bad('the elements must start with vertex, face; found %s' % [e[0] for e in elements])
    if any(e[1] for e in elements[2:]):
        raise bad('elements after the faces are not read (%s)' % [e[0] for e in elements[2:]])
    (_, n_v, vprops), (_, n_f, fprops) = elements[:2]
    fields = []
    for w in vprops:
        if w[0] == 'list' or len(w) != 2 or w[0] not in _PLY_SCALARS:
            raise bad('vertex property %r (scalar properties only)' % ' '.join(w))
        fields.append((w[1], _PLY_SCALARS[w[0]]))
    names = [n for n, _ in fields]
    if len(set(names)) != len(names):
        raise bad('a vertex property is declared twice')
    for axis in 'xyz':
        if axis not in names or dict(fields)[axis] not in ('<f4', '<f8'):
            raise bad('vertex property %s must be float or double' % axis)
    if len(fprops) != 1 or fprops[0][0] != 'list' or len(fprops[0]) != 4:
        raise bad('the face element must hold one list property, found %s' % [' '.join(w) for w in fprops])
    _, count_t, index_t, _ = fprops[0]
    if _PLY_SCALARS.get(count_t) != 'u1' or _PLY_SCALARS.get(index_t) not in ('<i4', '<u4'):
        raise bad('face list of %s count and %s indices (uchar count with int or uint indices only)' % (count_t, index_t))
    vt = np.dtype(fields)
    ft = np.dtype([('n', 'u1'), ('i', _PLY_SCALARS[index_t], (3,))])
    need = end + n_v * vt.itemsize + n_f * ft.itemsize
    if len(data) != need:
        raise bad('truncated, or a face that is not a triangle (%d bytes, %d expected for triangles)' % (len(data), need))
    rows = np.frombuffer(data, dtype=vt, count=n_v, offset=end)
    faces = np.frombuffer(data, dtype=ft, count=n_f, offset=end + n_v * vt.itemsize)
    if n_f and not (faces['n'] == 3).all():
        raise bad('a face that is not a triangle')
    idx = faces['i']
    if n_f and (int(idx.max()) >= 2 ** 31 or int(idx.min()) < 0 or int(idx.max()) >= n_v):
        raise bad('a face index outside the %d vertices' % n_v)
    verts = np.stack((rows['x'], rows['y'], rows['z']), axis=1).astype(np.float32).reshape(-1, 3)
    cols = None
    if all(c in names and dict(fields)[c] == 'u1' for c in ('red', 'green', 'blue')):
        cols = torch.from_numpy(np.ascontiguousarray(np.stack((rows['red'], rows['green'], rows['blue']), axis=1).reshape(-1, 3)))
    return TriangleMesh(torch.from_numpy(np.ascontiguousarray(verts)),
                        torch.from_numpy(np.ascontiguousarray(idx.astype(np.int32).reshape(-1, 3))), cols)
