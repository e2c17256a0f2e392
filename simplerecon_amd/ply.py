"""PLY reader for ground-truth meshes and point clouds, and the writer behind TriangleMesh.write_ply and
PointCloud.write_ply (host, numpy).

    read_ply(path) -> tsdf.TriangleMesh      when the file has a face element
                   -> point_cloud.PointCloud otherwise
    write_ply(path, columns, faces=None)     binary little-endian: per-vertex columns, optional triangles

Reads `binary_little_endian` and `ascii` files.  Vertex properties may have any scalar type: `x, y, z` are kept as fp32
and `red, green, blue` as uint8 for point clouds, as fp32 in [0, 1] (integer values / 255) for meshes; every other property (ScanNet's `alpha`, normals, ...) is skipped.
Faces are `list <uchar|char|ushort|short|int|uint> <int|uint> vertex_indices` (or `vertex_index`); triangles are taken
as they are and polygons with more vertices are fan-triangulated around their first vertex (v0, vi, vi+1).  Other
elements (edges, materials, ...) are skipped.  It reads everything TriangleMesh.write_ply and PointCloud.write_ply
write.  A header it cannot read raises ValueError naming the offending line, and so do face indices outside the vertex
range and files shorter than their header says.  Results are CPU tensors."""
import numpy as np
import torch

_SCALARS = {
    "char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1",
    "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
    "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
    "float": "f4", "float32": "f4", "double": "f8", "float64": "f8",
}
_NAMES = {"i1": "char", "u1": "uchar", "i2": "short", "u2": "ushort", "i4": "int", "u4": "uint", "f4": "float",
          "f8": "double"}


def write_ply(path, columns, faces=None):
    """Writes a binary little-endian PLY.  `columns` is the ordered list of per-vertex properties as (name, dtype, [V]
    array) with a little-endian numpy scalar dtype ("<f4", "u1", ...); `faces`, when given (an empty array included),
    is [F,3] int32 and becomes a `list uchar int vertex_indices` face element -- the layout trimesh writes."""
    n = len(columns[0][2])
    vrec = np.empty(n, dtype=[(name, dt) for name, dt, _ in columns])
    for name, _, values in columns:
        vrec[name] = values
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    header += [f"property {_NAMES[np.dtype(dt).str[1:]]} {name}" for name, dt, _ in columns]
    body = vrec.tobytes()
    if faces is not None:
        frec = np.empty(len(faces), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        frec["n"] = 3
        frec["i"] = faces
        header += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
        body += frec.tobytes()
    with open(path, "wb") as fh:
        fh.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        fh.write(body)


class _Element:
    def __init__(self, name, count):
        self.name = name
        self.count = count
        self.props = []   # (name, dtype) or (name, ("list", count dtype, item dtype))


def _parse_header(fh):
    first = fh.readline()
    if first.strip() != b"ply":
        raise ValueError(f"not a PLY file: first line {first[:40]!r}")
    fmt, elements = None, []
    while True:
        raw = fh.readline()
        if not raw:
            raise ValueError("PLY header has no end_header line")
        line = raw.decode("ascii", errors="replace").strip()
        words = line.split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            break
        if words[0] == "format":
            if len(words) != 3 or words[1] not in ("ascii", "binary_little_endian"):
                raise ValueError(f"unsupported PLY format line: {line!r} (ascii and binary_little_endian are read)")
            fmt = words[1]
        elif words[0] == "element":
            if len(words) != 3 or not words[2].isdigit():
                raise ValueError(f"bad PLY element line: {line!r}")
            elements.append(_Element(words[1], int(words[2])))
        elif words[0] == "property":
            if not elements:
                raise ValueError(f"PLY property before any element: {line!r}")
            if len(words) == 5 and words[1] == "list":
                if words[2] not in _SCALARS or words[3] not in _SCALARS:
                    raise ValueError(f"bad PLY list property: {line!r}")
                elements[-1].props.append((words[4], ("list", _SCALARS[words[2]], _SCALARS[words[3]])))
            elif len(words) == 3 and words[1] in _SCALARS:
                elements[-1].props.append((words[2], _SCALARS[words[1]]))
            else:
                raise ValueError(f"bad PLY property line: {line!r}")
        else:
            raise ValueError(f"unknown PLY header line: {line!r}")
    if fmt is None:
        raise ValueError("PLY header has no format line")
    return fmt, elements


def _has_list(el):
    return any(isinstance(t, tuple) for _, t in el.props)


def _read_binary(buf, pos, el):
    """Returns ({name: array, or a list of arrays for a list property}, new position) for one element."""
    if not _has_list(el):
        dt = np.dtype([(n, "<" + t) for n, t in el.props])
        end = pos + dt.itemsize * el.count
        if end > len(buf):
            raise ValueError(f"PLY file ends inside element {el.name!r}")
        rec = np.frombuffer(buf, dtype=dt, count=el.count, offset=pos)
        return {n: rec[n] for n, _ in el.props}, pos + dt.itemsize * el.count
    # elements with lists: fast path for one list whose count is the same for every row (all triangles, say)
    scalars = {n: [] for n, t in el.props if not isinstance(t, tuple)}
    if len(el.props) == 1:
        name, (_, ct, it) = el.props[0]
        cdt, idt = np.dtype("<" + ct), np.dtype("<" + it)
        if el.count == 0:
            return {name: np.zeros((0, 0), idt)}, pos
        if pos + cdt.itemsize > len(buf):
            raise ValueError(f"PLY file ends inside element {el.name!r}")
        k = int(np.frombuffer(buf, dtype=cdt, count=1, offset=pos)[0])
        row = np.dtype([("n", cdt), ("v", idt, (k,))])
        end = pos + row.itemsize * el.count
        if k > 0 and end <= len(buf):
            rec = np.frombuffer(buf, dtype=row, count=el.count, offset=pos)
            if (rec["n"] == k).all():
                return {name: rec["v"]}, end
    # general path: row by row
    lists = {n: [] for n, t in el.props if isinstance(t, tuple)}
    for _ in range(el.count):
        for n, t in el.props:
            if isinstance(t, tuple):
                cdt, idt = np.dtype("<" + t[1]), np.dtype("<" + t[2])
                if pos + cdt.itemsize > len(buf):
                    raise ValueError(f"PLY file ends inside element {el.name!r}")
                k = int(np.frombuffer(buf, dtype=cdt, count=1, offset=pos)[0])
                pos += cdt.itemsize
                if pos + idt.itemsize * k > len(buf):
                    raise ValueError(f"PLY file ends inside element {el.name!r}")
                lists[n].append(np.frombuffer(buf, dtype=idt, count=k, offset=pos))
                pos += idt.itemsize * k
            else:
                dt = np.dtype("<" + t)
                if pos + dt.itemsize > len(buf):
                    raise ValueError(f"PLY file ends inside element {el.name!r}")
                scalars[n].append(np.frombuffer(buf, dtype=dt, count=1, offset=pos)[0])
                pos += dt.itemsize
    out = {n: np.array(v) for n, v in scalars.items()}
    out.update(lists)
    return out, pos


def _read_ascii(lines, li, el):
    out = {n: [] for n, _ in el.props}
    for r in range(el.count):
        if li >= len(lines):
            raise ValueError(f"PLY file ends inside element {el.name!r}")
        words = lines[li].split()
        li += 1
        j = 0
        try:
            for n, t in el.props:
                if isinstance(t, tuple):
                    k = int(words[j])
                    out[n].append(np.array([float(w) for w in words[j + 1:j + 1 + k]]).astype(t[2]))
                    if len(out[n][-1]) != k:
                        raise IndexError
                    j += 1 + k
                else:
                    out[n].append(float(words[j]))
                    j += 1
        except (IndexError, ValueError):
            raise ValueError(f"bad PLY data line {li} in element {el.name!r}: {lines[li - 1][:80]!r}") from None
    res = {}
    for n, t in el.props:
        res[n] = out[n] if isinstance(t, tuple) else np.array(out[n], dtype=t)
    return res, li


def _triangles(faces, nverts, name):
    """[F,3] int64 from a [F,k] array or a list of index arrays (fan triangulation of polygons)."""
    if isinstance(faces, np.ndarray) and faces.ndim == 2 and faces.shape[1] in (0, 3):
        tri = faces.astype(np.int64).reshape(-1, 3)
    else:
        tris = []
        for f in faces:
            f = np.asarray(f, dtype=np.int64)
            if len(f) < 3:
                raise ValueError(f"{name}: a face with {len(f)} vertices")
            tris += [(f[0], f[i], f[i + 1]) for i in range(1, len(f) - 1)]
        tri = np.array(tris, dtype=np.int64).reshape(-1, 3)
    if tri.size and (tri.min() < 0 or tri.max() >= nverts):
        raise ValueError(f"{name}: face indices outside [0, {nverts}) (min {tri.min()}, max {tri.max()})")
    return tri


def read_ply(path):
    """Reads a PLY file: a CPU tsdf.TriangleMesh (vertices fp32, faces int32, normals None, colors [V,3] fp32 in [0, 1]
    when red / green / blue are present, else None) when it has a face element, else a CPU point_cloud.PointCloud (points fp32, colours uint8 when red / green / blue are present)."""
    from .point_cloud import PointCloud
    from .tsdf import TriangleMesh
    with open(path, "rb") as fh:
        fmt, elements = _parse_header(fh)
        body = fh.read()
    data = {}
    if fmt == "ascii":
        lines = [ln for ln in body.decode("ascii", errors="replace").splitlines() if ln.strip()]
        li = 0
        for el in elements:
            data[el.name], li = _read_ascii(lines, li, el)
    else:
        pos = 0
        for el in elements:
            data[el.name], pos = _read_binary(body, pos, el)
    if "vertex" not in data:
        raise ValueError(f"{path}: no vertex element")
    v = data["vertex"]
    for axis in "xyz":
        if axis not in v or isinstance(v[axis], list):
            raise ValueError(f"{path}: the vertex element has no scalar property {axis!r}")
    pts = np.stack([np.asarray(v[a], dtype=np.float32) for a in "xyz"], 1).reshape(-1, 3)
    if "face" in data:
        f = data["face"]
        key = "vertex_indices" if "vertex_indices" in f else ("vertex_index" if "vertex_index" in f else None)
        if key is None:
            raise ValueError(f"{path}: the face element has no vertex_indices list")
        tri = _triangles(f[key], len(pts), str(path))
        colors = None
        if all(c in v and not isinstance(v[c], list) for c in ("red", "green", "blue")):
            # integer colours are 0..255 (write_ply's uchar); float colours are taken as they are, in [0, 1]
            chans = [np.asarray(v[c]) for c in ("red", "green", "blue")]
            colors = torch.from_numpy(np.stack([a.astype(np.float32) / np.float32(255) if a.dtype.kind in "iu"
                                                else a.astype(np.float32) for a in chans], 1).reshape(-1, 3).copy())
        return TriangleMesh(torch.from_numpy(np.ascontiguousarray(pts)), torch.from_numpy(tri.astype(np.int32)),
                            colors=colors)
    cols = None
    if all(c in v and not isinstance(v[c], list) for c in ("red", "green", "blue")):
        cols = torch.from_numpy(np.stack([np.asarray(v[c]).astype(np.uint8) for c in ("red", "green", "blue")], 1)
                                .reshape(-1, 3).copy())
    return PointCloud(torch.from_numpy(np.ascontiguousarray(pts)), cols)
