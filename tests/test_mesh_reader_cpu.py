"""CPU: the vectorised face block of extras.mesh_sampling.read_ply_mesh (binary PLY whose faces all have one vertex count)
against the per-face loop it falls back to - little- and big-endian, triangles, quads, hexagons, extra face properties before
the next element - and the loop taken for mixed face sizes; the shared candidate / ray-offset helpers against what
sample_mesh_points and points_in_mesh did inline."""
import numpy as np
import pytest

from neuma_amd.extras import mesh_sampling as mesh


def _write_binary_ply(path, verts, faces, endian="<", count_type=("uchar", "u1"), index_type=("int", "i4"), extra=(),
                      trailing=False):
    """faces: list of index lists (any sizes); extra: ((ply type, numpy type, name), ...) per-face properties after the list."""
    hdr = ["ply", f"format {'binary_little_endian' if endian == '<' else 'binary_big_endian'} 1.0",
           f"element vertex {len(verts)}", "property double x", "property double y", "property double z",
           f"element face {len(faces)}", f"property list {count_type[0]} {index_type[0]} vertex_indices"]
    hdr += [f"property {pt} {name}" for pt, _, name in extra]
    if trailing:
        hdr += ["element edge 1", "property int vertex1", "property int vertex2"]
    hdr.append("end_header")
    body = bytearray(np.asarray(verts, dtype=endian + "f8").tobytes())
    for i, f in enumerate(faces):
        body += np.array([len(f)], dtype=endian + count_type[1]).tobytes()
        body += np.asarray(f, dtype=endian + index_type[1]).tobytes()
        for _, nt, _ in extra:
            body += np.array([i % 7], dtype=endian + nt).tobytes()
    if trailing:
        body += np.array([0, 1], dtype=endian + "i4").tobytes()
    path.write_bytes(("\n".join(hdr) + "\n").encode() + bytes(body))


def _read_by_loop(path, monkeypatch):
    with monkeypatch.context() as m:
        m.setattr(mesh, "_ply_faces_uniform", lambda *a: None)
        return mesh.read_ply_mesh(path)


def _faces(rng, n, k, nv):
    return [list(rng.integers(0, nv, k)) for _ in range(n)]


@pytest.mark.parametrize("endian", ["<", ">"])
@pytest.mark.parametrize("k", [3, 4, 6])
@pytest.mark.parametrize("extra", [(), (("uchar", "u1", "flags"), ("float", "f4", "quality"), ("double", "f8", "w"))])
def test_uniform_faces_read_in_one_block_match_the_loop(tmp_path, monkeypatch, endian, k, extra):
    rng = np.random.default_rng(k)
    verts = rng.normal(size=(50, 3))
    faces = _faces(rng, 200, k, len(verts))
    path = tmp_path / "m.ply"
    _write_binary_ply(path, verts, faces, endian=endian, extra=extra, trailing=True,
                      index_type=("uint", "u4") if k == 4 else ("int", "i4"))
    calls = []
    fast = mesh._ply_faces_uniform
    monkeypatch.setattr(mesh, "_ply_faces_uniform", lambda *a: calls.append(fast(*a)) or calls[-1])
    v, t = mesh.read_ply_mesh(path)
    assert calls and calls[0] is not None                              # the block path answered
    monkeypatch.undo()
    v2, t2 = _read_by_loop(path, monkeypatch)
    assert v.dtype == v2.dtype == np.float64 and t.dtype == t2.dtype == np.int64
    assert np.array_equal(v, v2) and np.array_equal(t, t2) and t.shape == (200 * (k - 2), 3)
    assert np.array_equal(v, verts)
    expect = [(f[0], f[i], f[i + 1]) for f in faces for i in range(1, k - 1)]
    assert np.array_equal(t, np.asarray(expect, dtype=np.int64))


@pytest.mark.parametrize("endian", ["<", ">"])
def test_mixed_face_sizes_take_the_loop(tmp_path, monkeypatch, endian):
    rng = np.random.default_rng(1)
    verts = rng.normal(size=(30, 3))
    faces = _faces(rng, 20, 3, 30) + _faces(rng, 5, 4, 30) + _faces(rng, 3, 3, 30)
    path = tmp_path / "mixed.ply"
    _write_binary_ply(path, verts, faces, endian=endian, count_type=("uint8", "u1"), extra=(("short", "i2", "s"),))
    calls = []
    fast = mesh._ply_faces_uniform
    monkeypatch.setattr(mesh, "_ply_faces_uniform", lambda *a: calls.append(fast(*a)) or calls[-1])
    v, t = mesh.read_ply_mesh(path)
    assert calls == [None]
    expect = [(f[0], f[i], f[i + 1]) for f in faces for i in range(1, len(f) - 1)]
    assert np.array_equal(t, np.asarray(expect, dtype=np.int64)) and np.array_equal(v, verts)


def test_ascii_and_empty_face_blocks_are_unchanged(tmp_path):
    path = tmp_path / "a.ply"
    path.write_text("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                    "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    v, t = mesh.read_ply_mesh(path)
    assert t.tolist() == [[0, 1, 2], [0, 2, 3]] and v.shape == (4, 3)
    path = tmp_path / "e.ply"
    _write_binary_ply(path, np.zeros((3, 3)), [])
    v, t = mesh.read_ply_mesh(path)
    assert t.shape == (0, 3) and t.dtype == np.int64


def test_shared_helpers_reproduce_the_inline_candidates_and_offset():
    rng = np.random.default_rng(0)
    verts = rng.normal(size=(40, 3)) * [2.0, 1.0, 0.5] + 3.0
    lo, hi = verts.min(0), verts.max(0)
    h = float((hi - lo).max()) / 17
    axes = [np.arange(lo[k] + 0.5 * h, hi[k], h) for k in range(3)]
    lattice = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    assert np.array_equal(mesh.mesh_candidate_points(verts, "volumetric", 17), lattice)
    uni = lo + (hi - lo) * np.random.default_rng(5).random((9 ** 3, 3))
    assert np.array_equal(mesh.mesh_candidate_points(verts, "uniform", 9, seed=5), uni)
    with pytest.raises(ValueError):
        mesh.mesh_candidate_points(verts, "surface", 9)
    span = float(np.abs(verts).max())
    assert np.array_equal(mesh.ray_offset_points(lattice, verts), lattice + np.array([1.2345678e-7, 2.7182818e-7, 0.0]) * span)
