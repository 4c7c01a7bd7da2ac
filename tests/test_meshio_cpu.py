"""CPU: nsdp_amd/meshio.py.  Every accepted form of every format from files written by hand here, compared with the arrays they
were meant to hold; the writer's round trip; every refusal, with the file named."""
import struct

import numpy as np
import pytest

from nsdp_amd import meshio

VERTS = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [1.0, 1.25, 0.0], [0.0, 1.0, -2.5e-3], [0.5, 0.5, 1e3]])
# a triangle, a quad (fanned from its first corner) and a pentagon
POLYGONS = [[0, 1, 2], [0, 1, 2, 3], [4, 3, 2, 1, 0]]
FANNED = np.array([[0, 1, 2], [0, 1, 2], [0, 2, 3], [4, 3, 2], [4, 2, 1], [4, 1, 0]], dtype=np.int32)


def _check(path, verts=VERTS, faces=FANNED):
    v, f = meshio.read_mesh(path)
    assert v.dtype == np.float64 and f.dtype == np.int32 and v.flags.c_contiguous and f.flags.c_contiguous
    assert np.array_equal(v, verts), (v, verts)
    assert np.array_equal(f, faces), (f, faces)


def _vlines(extra=""):
    return "".join("v {!r} {!r} {!r}{}\n".format(*[float(x) for x in v], extra) for v in VERTS)


# ------------------------------------------------------------------------------------------------------------------ .obj
def test_obj_index_forms_negative_indices_and_a_quad(tmp_path):
    p = tmp_path / "forms.obj"
    p.write_text("# a comment\nmtllib x.mtl\n" + _vlines() + "vt 0 0\nvn 0 0 1\ng part\n"
                 "f 1 2 3\n"                             # a
                 "f 1/1 2/1 3/1 4/1\n"                   # a/b, a quad
                 "f 5/1/1 4//1 3/1 2//1 1/1/1\n"         # a/b/c and a//c mixed, a pentagon
                 "s off\n")
    _check(str(p))
    p = tmp_path / "negative.obj"
    p.write_text(_vlines() + "f -5 -4 -3\nf -5//1 -4//1 -3//1 -2//1\nf -1 -2 -3 -4 -5\n")
    _check(str(p))
    # negative indices count back from the vertices read SO FAR; colours after the coordinates are ignored
    p = tmp_path / "interleaved.obj"
    lines = _vlines(" 0.5 0.25 1.0").splitlines()
    p.write_text("\n".join(lines[:3]) + "\nf -3 -2 -1\n" + "\n".join(lines[3:]) + "\nf 1 2 3 4\nf -1 -2 -3 -4 -5\n")
    _check(str(p))
    # statements of different lengths (one vertex with a colour, the others without)
    p = tmp_path / "ragged.obj"
    p.write_text("\n".join(lines[:1]) + "\n" + "".join(_vlines().splitlines(True)[1:]) + "f 1 2 3\nf 1 2 3 4\nf 5 4 3 2 1\n")
    _check(str(p))
    # ... and ragged files whose TOTAL number count divides by the vertex count (6 + 3 + 3 = 12 numbers over 3 vertices): the
    # widths are judged statement by statement, never from the total
    p = tmp_path / "ragged_dividing.obj"
    p.write_text("v 1 2 3 0.1 0.2 0.3\nv 4 5 6\nv 7 8 9\nf 1 2 3\n")
    _check(str(p), np.array([[1.0, 2, 3], [4, 5, 6], [7, 8, 9]]), np.array([[0, 1, 2]], dtype=np.int32))
    p = tmp_path / "ragged_dividing_w.obj"                                   # 4 + 4 + 3 + 3 + 6 = 20 numbers over 5 vertices
    plain = _vlines().splitlines()
    p.write_text("\n".join([plain[0] + " 1.0", plain[1] + " 1.0", plain[2], plain[3], plain[4] + " 0.5 0.25 1.0"])
                 + "\nf 1 2 3\nf 1 2 3 4\nf 5 4 3 2 1\n")
    _check(str(p))
    # a trailing backslash continues a statement
    p = tmp_path / "continued.obj"
    p.write_text(_vlines().replace(" 1.25", " \\\n 1.25") + "f 1 2 \\\n3\nf 1 2 3 \\\n 4\nf 5 4 3 2 1\n")
    assert "\\\n" in p.read_text()
    _check(str(p))


# ------------------------------------------------------------------------------------------------------------------ .ply
def _ply_header(fmt, vertex_props, n_faces, list_types, extra_element=""):
    return ("ply\nformat {} 1.0\ncomment made by hand\n{}element vertex {}\n{}element face {}\nproperty list {} {} vertex_indices\n"
            "end_header\n").format(fmt, extra_element, len(VERTS), "".join(f"property {t} {n}\n" for t, n in vertex_props), n_faces,
                                   *list_types)


def test_ply_ascii_with_extra_properties_and_mixed_polygons(tmp_path):
    props = [("uchar", "red"), ("float", "x"), ("double", "y"), ("int", "flag"), ("float", "z")]
    body = "".join("7 {!r} {!r} -3 {!r}\n".format(*[float(x) for x in v]) for v in VERTS)
    body += "".join("{} {}\n".format(len(p), " ".join(map(str, p))) for p in POLYGONS)
    p = tmp_path / "ascii.ply"
    p.write_text(_ply_header("ascii", props, 3, ("uchar", "int")) + body)
    _check(str(p))
    # triangles only: the reader's path without a walk; an element of scalars in front is skipped
    p = tmp_path / "triangles.ply"
    p.write_text(_ply_header("ascii", [("float", "x"), ("float", "y"), ("float", "z")], len(FANNED), ("uint8", "uint32"),
                             "element camera 2\nproperty float a\nproperty int b\n") + "0.5 1\n0.25 2\n"
                 + "".join("{!r} {!r} {!r}\n".format(*[float(x) for x in v]) for v in VERTS)
                 + "".join("3 {} {} {}\n".format(*t) for t in FANNED))
    _check(str(p))


@pytest.mark.parametrize("count_type,index_type", [("uchar", "int"), ("ushort", "uint"), ("int", "short"), ("uint8", "uchar")])
@pytest.mark.parametrize("polygons", [POLYGONS, FANNED.tolist()])
def test_ply_binary_with_extra_properties_and_list_types(tmp_path, count_type, index_type, polygons):
    codes = {"uchar": "B", "uint8": "B", "ushort": "H", "int": "i", "uint": "I", "short": "h"}
    props = [("double", "x"), ("short", "quality"), ("double", "z"), ("uchar", "alpha"), ("double", "y")]
    body = b"".join(struct.pack("<dhdBd", v[0], -7, v[2], 255, v[1]) for v in VERTS)
    for poly in polygons:
        body += struct.pack("<" + codes[count_type], len(poly)) + struct.pack("<%d%s" % (len(poly), codes[index_type]), *poly)
    p = tmp_path / "binary.ply"
    p.write_bytes(_ply_header("binary_little_endian", props, len(polygons), (count_type, index_type)).encode() + body)
    _check(str(p))


def test_ply_elements_after_the_faces_are_not_read(tmp_path):
    props = [("float", "x"), ("float", "y"), ("float", "z")]
    head = _ply_header("binary_little_endian", props, 1, ("uchar", "int")).replace(
        "end_header\n", "element edge 2\nproperty int a\nproperty int b\nelement strips 1\nproperty list int int strip\nend_header\n")
    body = VERTS.astype(np.float32).tobytes() + struct.pack("<B3i", 3, 0, 1, 2) + struct.pack("<4i", 0, 1, 1, 2) + struct.pack("<4i", 3, 0, 1, 2)
    p = tmp_path / "trailing.ply"
    p.write_bytes(head.encode() + body)
    _check(str(p), VERTS.astype(np.float32).astype(np.float64), FANNED[:1])
    # in FRONT of the faces such an element cannot be skipped: refused, with the file and the element named
    head = _ply_header("ascii", props, 1, ("uchar", "int"), "element strips 1\nproperty list int int strip\n")
    p = tmp_path / "leading.ply"
    p.write_text(head + "3 0 1 2\n" + "".join("{} {} {}\n".format(*v) for v in VERTS) + "3 0 1 2\n")
    with pytest.raises(meshio.MeshError, match="leading.ply: element 'strips' in front"):
        meshio.read_mesh(str(p))


def test_ply_float_vertices_are_widened_exactly(tmp_path):
    v32 = VERTS.astype(np.float32) * np.float32(1.1)
    p = tmp_path / "f32.ply"
    p.write_bytes(_ply_header("binary_little_endian", [("float", "x"), ("float", "y"), ("float", "z")], 1, ("uchar", "int")).encode()
                  + v32.tobytes() + struct.pack("<B3i", 3, 0, 1, 2))
    _check(str(p), v32.astype(np.float64), FANNED[:1])


# ------------------------------------------------------------------------------------------------------------------ .off
def test_off_both_header_forms(tmp_path):
    body = "".join("{!r} {!r} {!r}\n".format(*[float(x) for x in v]) for v in VERTS)
    body += "".join("{} {}\n".format(len(p), " ".join(map(str, p))) for p in POLYGONS)
    (tmp_path / "two_lines.off").write_text("OFF\n# counts on their own line\n5 3 0\n" + body)
    (tmp_path / "one_line.off").write_text("OFF 5 3 0\n" + body)
    _check(str(tmp_path / "two_lines.off"))
    _check(str(tmp_path / "one_line.off"))


# ------------------------------------------------------------------------------------------------------------------ writer
def test_written_meshes_read_back(tmp_path):
    g = np.random.RandomState(1)
    verts = (g.rand(50, 3) - 0.5).astype(np.float32)
    faces = g.randint(0, 50, size=(80, 3)).astype(np.int32)
    colors = g.randint(0, 256, size=(50, 3)).astype(np.uint8)
    for name, kw in (("plain.ply", {}), ("coloured.ply", {"colors": colors})):
        meshio.write_mesh(str(tmp_path / name), verts, faces, **kw)
        v, f = meshio.read_mesh(str(tmp_path / name))
        assert np.array_equal(v.astype(np.float32), verts) and np.array_equal(v, verts.astype(np.float64))      # exact for fp32
        assert np.array_equal(f, faces)
    raw = (tmp_path / "coloured.ply").read_bytes()
    assert b"property uchar red" in raw and raw.endswith(struct.pack("<B3i", 3, *faces[-1]))
    meshio.write_mesh(str(tmp_path / "double.ply"), verts.astype(np.float64) / 3.0, faces)
    assert np.array_equal(meshio.read_mesh(str(tmp_path / "double.ply"))[0], verts.astype(np.float64) / 3.0)
    for name, kw in (("plain.obj", {}), ("coloured.obj", {"colors": colors})):
        meshio.write_mesh(str(tmp_path / name), verts, faces, **kw)
        v, f = meshio.read_mesh(str(tmp_path / name))
        assert np.array_equal(v.astype(np.float32), verts) and np.array_equal(f, faces)     # nine digits name one fp32 number
    meshio.write_mesh(str(tmp_path / "double.obj"), verts.astype(np.float64) / 3.0, faces)
    assert np.array_equal(meshio.read_mesh(str(tmp_path / "double.obj"))[0], verts.astype(np.float64) / 3.0)
    with pytest.raises(meshio.MeshError, match="mesh.stl"):
        meshio.write_mesh(str(tmp_path / "mesh.stl"), verts, faces)
    with pytest.raises(meshio.MeshError, match="colors"):
        meshio.write_mesh(str(tmp_path / "c.ply"), verts, faces, colors=colors[:10])


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_names_the_file_and_the_reason(tmp_path):
    def refused(name, text, reason, binary=False):
        p = tmp_path / name
        p.write_bytes(text) if binary else p.write_text(text)
        with pytest.raises(meshio.MeshError, match=reason) as e:
            meshio.read_mesh(str(p))
        assert name in str(e.value) and isinstance(e.value, ValueError)

    refused("beyond.obj", _vlines() + "f 1 2 6\n", r"outside \[0, 5\)")
    refused("zero.obj", _vlines() + "f 0 1 2\n", r"outside \[0, 5\)")
    refused("far_back.obj", _vlines() + "f -6 1 2\n", r"outside \[0, 5\)")
    refused("line.obj", _vlines() + "f 1 2 3\nf 1 2\n", "face 1 has 2 corners, fewer than three")
    refused("no_vertices.obj", "f 1 2 3\n", "no vertices")
    refused("no_faces.obj", _vlines(), "no faces")
    refused("empty.off", "OFF\n0 0 0\n", "no vertices")
    refused("short.off", "OFF 5 3 0\n0 0 0\n", "ends inside")
    refused("beyond.off", "OFF 3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 3\n", r"outside \[0, 3\)")
    refused("point.off", "OFF 3 1 0\n0 0 0\n1 0 0\n0 1 0\n1 0\n", "fewer than three")
    refused("mesh.stl", "solid\n", "unknown extension '.stl'")
    header = "ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n"
    refused("big.ply", header, "binary_big_endian")
    refused("no_faces.ply", _ply_header("ascii", [("float", "x"), ("float", "y"), ("float", "z")], 0, ("uchar", "int"))
            + "".join("{} {} {}\n".format(*v) for v in VERTS), "no faces")
    refused("beyond.ply", _ply_header("binary_little_endian", [("float", "x"), ("float", "y"), ("float", "z")], 1, ("uchar", "int")).encode()
            + VERTS.astype(np.float32).tobytes() + struct.pack("<B3i", 3, 0, 1, -1), r"outside \[0, 5\)", binary=True)
    refused("cut.ply", _ply_header("binary_little_endian", [("float", "x"), ("float", "y"), ("float", "z")], 2, ("uchar", "int")).encode()
            + VERTS.astype(np.float32).tobytes() + struct.pack("<B3i", 3, 0, 1, 2), "ends inside", binary=True)
    refused("no_xyz.ply", _ply_header("ascii", [("float", "x"), ("float", "y")], 0, ("uchar", "int")) + "0 0\n" * 5, "no x, y, z")
    with pytest.raises(meshio.MeshError, match="missing file .*nothing.obj"):
        meshio.read_mesh(str(tmp_path / "nothing.obj"))
