"""The readers and writers of the reference's utils/io_util.py under its names and return shapes, on numpy and the standard library alone
(the reference goes through the plyfile package; its termcolor helpers are not provided).

  read_ply, read_label_ply, read_color_ply   the named properties of a PLY file's FIRST element; everything behind that element -- ScanNet's
                                             face element with its list property -- is ignored, and so are properties nobody asks for (alpha)
  read_ply_faces                             the triangles of the `face` element behind the first element, (F, 3) int32
  write_mesh_ply                             x y z as f4 and a face element behind them, so that tests have meshes to read
  read_txt, read_label_txt                   lines, and one integer per line
  write_ply, write_color_ply                 ASCII (text=True, the reference's default) or binary little-endian PLY with the reference's
                                             property lists: x y z as f4, red green blue as u1, and the element comment `vertices`
  write_label_txt                            one decimal integer per line, the bytes of the reference's '{0}\\n'.format(label[i])

The reader takes `format ascii 1.0` and `format binary_little_endian 1.0`, comment / obj_info lines anywhere in the header and every scalar
property type of the format.  binary_big_endian, or a list property inside the first element, raises ValueError naming the file.

Floats are written as '%.9g': nine significant digits determine a float32, so the text reads back to the identical float32 (-0.0 included).
plyfile's own number formatting is not reproduced: byte identity with the files the reference writes is NOT claimed.  What holds is the round
trip, and that the reader takes both encodings."""
import numpy as np

__all__ = ["read_ply", "read_label_ply", "read_color_ply", "read_ply_faces", "read_txt", "read_label_txt", "write_ply", "write_color_ply",
           "write_mesh_ply", "write_label_txt"]

_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
          "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}
_NAMES = {"f4": "float", "u1": "uchar"}


def _first_element(filename):
    """-> a structured array of the first element's rows, fields by property name"""
    with open(filename, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("%s: not a PLY file (no 'ply' ... 'end_header')" % filename)
    body = data.find(b"\n", end) + 1
    if body <= 0:
        raise ValueError("%s: the header's last line does not end" % filename)
    fmt, count, fields, elements = None, 0, [], 0
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        words = line.split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "format":
            fmt = words[1] if len(words) > 1 else ""
        elif words[0] == "element":
            elements += 1
            if elements > 1:
                break                                                             # nothing behind the first element is read
            if len(words) != 3:
                raise ValueError("%s: malformed header line %r" % (filename, line))
            count = int(words[2])
        elif words[0] == "property" and elements == 1:
            if len(words) > 1 and words[1] == "list":
                raise ValueError("%s: the first element has a list property (%r): only scalar properties are read" % (filename, line))
            if len(words) != 3 or words[1] not in _TYPES:
                raise ValueError("%s: malformed header line %r" % (filename, line))
            fields.append((words[2], _TYPES[words[1]]))
        elif words[0] != "property":
            raise ValueError("%s: unknown header line %r" % (filename, line))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("%s: format %r is not read (ascii and binary_little_endian are)" % (filename, fmt))
    if elements == 0 or not fields or count < 0:
        raise ValueError("%s: the header declares no element with properties" % filename)
    if fmt == "binary_little_endian":
        dtype = np.dtype([(name, "<" + kind) for name, kind in fields])
        if len(data) - body < count * dtype.itemsize:
            raise ValueError("%s: %d rows of %d bytes declared, %d bytes present" % (filename, count, dtype.itemsize, len(data) - body))
        return np.frombuffer(data, dtype=dtype, count=count, offset=body)
    rows = data[body:].split(b"\n", count)[:count]
    values = np.array(b" ".join(rows).split(), dtype=np.float64)                # every scalar type of the format is exact in float64
    if len(rows) != count or values.size != count * len(fields):
        raise ValueError("%s: %d rows of %d numbers declared, %d numbers present" % (filename, count, len(fields), values.size))
    values = values.reshape(count, len(fields))
    out = np.empty(count, dtype=np.dtype(fields))
    for at, (name, _) in enumerate(fields):
        out[name] = values[:, at]                                                 # 9 digits -> float64 -> float32 is the float32 they name
    return out


def _columns(filename, names):
    rows = _first_element(filename)
    missing = [name for name in names if name not in rows.dtype.names]
    if missing:
        raise ValueError("%s: the first element has no property %s (it has %s)" % (filename, missing, list(rows.dtype.names)))
    return [np.ascontiguousarray(rows[name]) for name in names]


def read_ply(filename):
    """-> (n, 3) of x, y, z"""
    return np.stack(_columns(filename, ("x", "y", "z")), axis=1)


def read_label_ply(filename):
    """-> (n, 3) of x, y, z and (n,) label in the file's type"""
    x, y, z, label = _columns(filename, ("x", "y", "z", "label"))
    return np.stack([x, y, z], axis=1), label


def read_color_ply(filename):
    """-> (n, 6) of x, y, z, red, green, blue in the type numpy promotes them to (float32 for ScanNet's float and uchar)"""
    return np.stack(_columns(filename, ("x", "y", "z", "red", "green", "blue")), axis=1)


_COUNT_TYPES, _INDEX_TYPES = ("uchar", "uint8"), ("int", "int32", "uint", "uint32")


def read_ply_faces(filename):
    """-> (F, 3) int32: the triangles of the `face` element that follows the file's first (vertex) element, ScanNet's
    <scan>_vh_clean_2.ply.  The face element must hold one list property, its count uchar / uint8 and its indices int / int32 / uint /
    uint32; ascii and binary_little_endian.  Raises ValueError for a file without such an element, a face that is not a triangle, an index
    beyond int32, or a file that ends before the faces do."""
    with open(filename, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("%s: not a PLY file (no 'ply' ... 'end_header')" % filename)
    body = data.find(b"\n", end) + 1
    if body <= 0:
        raise ValueError("%s: the header's last line does not end" % filename)
    fmt, elements = None, []                                                      # [name, count, [property words]]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        words = line.split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "format":
            fmt = words[1] if len(words) > 1 else ""
        elif words[0] == "element" and len(words) == 3:
            elements.append([words[1], int(words[2]), []])
        elif words[0] == "property" and elements:
            elements[-1][2].append(words[1:])
        else:
            raise ValueError("%s: unknown header line %r" % (filename, line))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("%s: format %r is not read (ascii and binary_little_endian are)" % (filename, fmt))
    if len(elements) < 2 or elements[1][0] != "face":
        raise ValueError("%s: no face element behind the first element" % filename)
    (_, nvert, vprops), (_, count, fprops) = elements[:2]
    if nvert < 0 or count < 0 or any(len(p) != 2 or p[0] not in _TYPES for p in vprops):
        raise ValueError("%s: the first element is not one of scalar properties" % filename)
    if len(fprops) != 1 or len(fprops[0]) != 4 or fprops[0][0] != "list" or fprops[0][1] not in _COUNT_TYPES or fprops[0][2] not in _INDEX_TYPES:
        raise ValueError("%s: the face element must hold one list property, uchar counts of int or uint indices, got %r" % (filename, fprops))
    kind = _TYPES[fprops[0][2]]
    if fmt == "binary_little_endian":
        at = body + nvert * sum(np.dtype(_TYPES[p[0]]).itemsize for p in vprops)
        rows = np.dtype([("n", "u1"), ("i", "<" + kind, (3,))])                   # 13 bytes, unpadded
        have = max(len(data) - at, 0)
        whole = np.frombuffer(data, dtype=rows, count=min(count, have // rows.itemsize), offset=min(at, len(data)))
        if np.any(whole["n"] != 3):
            raise ValueError("%s: face %d is not a triangle" % (filename, int(np.flatnonzero(whole["n"] != 3)[0])))
        if whole.shape[0] != count:
            raise ValueError("%s: %d faces of %d bytes declared, %d bytes present" % (filename, count, rows.itemsize, have))
        idx = whole["i"].astype(np.int64)
    else:
        lines = data[body:].split(b"\n", nvert + count)
        if len(lines) < nvert + count:
            raise ValueError("%s: %d vertices and %d faces declared, %d lines present" % (filename, nvert, count, len(lines)))
        cells = [line.split() for line in lines[nvert:nvert + count]]
        for at, row in enumerate(cells):
            if not row:
                raise ValueError("%s: %d faces declared, %d present" % (filename, count, at))
            if row[0] != b"3" or len(row) != 4:
                raise ValueError("%s: face %d is not a triangle" % (filename, at))
        idx = np.array(cells, dtype=np.int64).reshape(count, 4)[:, 1:]
    if idx.size and (idx.min() < -(1 << 31) or idx.max() >= 1 << 31):
        raise ValueError("%s: a vertex index does not fit int32" % filename)
    return np.ascontiguousarray(idx.astype(np.int32))


def read_txt(filename):
    """-> the stripped lines, a list"""
    with open(filename) as f:
        return [line.strip() for line in f]


def read_label_txt(filename):
    """-> one integer per line, an array"""
    with open(filename) as f:
        return np.array([int(line.strip()) for line in f])


def _write_vertices(vertex, filename, text):
    header = ["ply", "format %s 1.0" % ("ascii" if text else "binary_little_endian"), "comment vertices", "element vertex %d" % vertex.shape[0]]
    header += ["property %s %s" % (_NAMES[vertex.dtype[name].str[1:]], name) for name in vertex.dtype.names]
    with open(filename, "wb") as f:
        f.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        if not text:
            f.write(vertex.tobytes())
            return
        columns = [vertex[name].tolist() for name in vertex.dtype.names]
        kinds = ["%.9g" if vertex.dtype[name].kind == "f" else "%d" for name in vertex.dtype.names]
        line = " ".join(kinds) + "\n"
        f.write("".join(line % row for row in zip(*columns)).encode("ascii"))


def _vertex_array(points, fields):
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] < len(fields):
        raise ValueError("expected (n, %d) points, got %s" % (len(fields), points.shape))
    vertex = np.empty(points.shape[0], dtype=[(name, "<" + kind) for name, kind in fields])
    for at, (name, _) in enumerate(fields):
        vertex[name] = points[:, at]
    return vertex


def write_ply(points, filename, text=True):
    """points (n, 3) -> a PLY file of x, y, z as f4"""
    _write_vertices(_vertex_array(points, (("x", "f4"), ("y", "f4"), ("z", "f4"))), filename, text)


def write_color_ply(points, filename, text=True):
    """points (n, 6) of x, y, z, red, green, blue -> a PLY file of x, y, z as f4 and red, green, blue as u1"""
    _write_vertices(_vertex_array(points, (("x", "f4"), ("y", "f4"), ("z", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"))), filename, text)


def write_mesh_ply(points, faces, filename, text=True, index_type="int"):
    """points (n, 3), faces (F, 3) integers -> a PLY file of x, y, z as f4 and a face element `property list uchar <index_type>
    vertex_indices` behind it (index_type "int" or "uint"), ScanNet's layout without its colours"""
    vertex = _vertex_array(points, (("x", "f4"), ("y", "f4"), ("z", "f4")))
    faces = np.asarray(faces)
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.dtype.kind not in "iu":
        raise ValueError("expected (F, 3) integer faces, got %s %s" % (faces.shape, faces.dtype))
    if index_type not in ("int", "uint"):
        raise ValueError("index_type must be 'int' or 'uint', got %r" % (index_type,))
    header = ["ply", "format %s 1.0" % ("ascii" if text else "binary_little_endian"), "comment vertices", "element vertex %d" % vertex.shape[0]]
    header += ["property float %s" % name for name in vertex.dtype.names]
    header += ["element face %d" % faces.shape[0], "property list uchar %s vertex_indices" % index_type, "end_header"]
    with open(filename, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        if text:
            f.write("".join("%.9g %.9g %.9g\n" % row for row in zip(*(vertex[name].tolist() for name in vertex.dtype.names))).encode("ascii"))
            f.write("".join("3 %d %d %d\n" % tuple(row) for row in faces.tolist()).encode("ascii"))
            return
        rows = np.empty(faces.shape[0], dtype=[("n", "u1"), ("i", "<" + _TYPES[index_type], (3,))])
        rows["n"] = 3
        rows["i"] = faces
        f.write(vertex.tobytes())
        f.write(rows.tobytes())


def write_label_txt(label, filename):
    """one decimal integer per line"""
    label = np.asarray(label).reshape(-1)
    with open(filename, "w") as f:
        f.write("".join("%d\n" % v for v in label.tolist()))
