"""CPU tests of attribute shading's host side: per-corner vt / vn parsing (and that it changes nothing else the OBJ reader returns), map_Kd
texture slots, PPM / TGA decoding with the magenta fallback, argument errors before any device work, and hand-worked cases of
tests/attr_ref.py (bilinear sampling, repeat addressing, the sRGB table, the non-finite uv rule, the texture after the ambient term)."""
import re
import struct

import numpy as np
import pytest

import attr_ref
import render_ref

F = np.float32


def strip_attributes(text):
    """the same OBJ without vt / vn lines and with every face corner reduced to its position index"""
    out = []
    for line in text.split("\n"):
        s = line.lstrip(" \t")
        if re.match(r"v[tn][ \t]", s):
            out.append("# attribute line")      # keeps the line numbers of error messages
            continue
        if re.match(r"f[ \t]", s):
            line = re.sub(r"(?<=[ \t])([+-]?\d+)/\S*", r"\1", line)
        out.append(line)
    return "\n".join(out)


def load(vx, path):
    try:
        m = vx.Mesh.load_obj(str(path))
    except vx.VxError as e:
        return None, (e.status, e.message)
    return m, None


def same_as_stripped(vx, tmp_path, text, name="a.obj"):
    p, q = tmp_path / name, tmp_path / ("stripped_" + name)
    p.write_text(text)
    q.write_text(strip_attributes(text))
    a, ea = load(vx, p)
    b, eb = load(vx, q)
    assert ea == eb
    if a is None:
        return None
    for x, y in zip(a.host_arrays(), b.host_arrays()):
        assert np.array_equal(x, y)
    ra, ia = a.materials()
    rb, ib = b.materials()
    assert ra.tobytes() == rb.tobytes() and (ia is None) == (ib is None) and (ia is None or np.array_equal(ia, ib))
    assert b.corner_normals() is None and b.corner_uvs() is None
    return a


QUAD = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\n"


def test_fan_corners_and_flip(vx, tmp_path):
    text = QUAD + "vt 0.25 0.5\nvt 0.75 0.125\nvt 1 1\nvt 0 1\nvn 0 0 1\nvn 0 1 0\nvn 1 0 0\nvn 0.5 0.5 0\n" \
                  "f 1/1/1 2/2/2 3/3/3 4/4/4\n"
    m = same_as_stripped(vx, tmp_path, text)
    _, t = m.host_arrays()
    assert t.tolist() == [[0, 1, 2], [0, 2, 3]]                  # fan (0, k-1, k)
    n, uv = m.corner_normals(), m.corner_uvs()
    vns = F([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.5, 0.5, 0]])
    vts = F([[0.25, 0.5], [0.75, 0.125], [1, 1], [0, 1]])
    vts[:, 1] = F(1) - vts[:, 1]
    assert np.array_equal(n, vns[[[0, 1, 2], [0, 2, 3]]])
    assert np.array_equal(uv, vts[[[0, 1, 2], [0, 2, 3]]])


def test_negative_and_mixed_corners(vx, tmp_path):
    text = QUAD + "vt 0.5 0.25\nvn 0 0 1\nvn 1 0 0\nf -4//-2 -3/1 -2//-1\nf 1/-1/2 3 4//1\n"
    m = same_as_stripped(vx, tmp_path, text)
    n, uv = m.corner_normals(), m.corner_uvs()
    assert np.array_equal(n[0], F([[0, 0, 1], [0, 0, 0], [1, 0, 0]]))
    assert np.array_equal(uv[0], F([[0, 0], [0.5, 0.75], [0, 0]]))
    assert np.array_equal(n[1], F([[1, 0, 0], [0, 0, 0], [0, 0, 1]]))
    assert np.array_equal(uv[1], F([[0.5, 0.75], [0, 0], [0, 0]]))


def test_unreferenced_and_out_of_range(vx, tmp_path):
    m = same_as_stripped(vx, tmp_path, QUAD + "vn 0 0 1\nf 1 2 3\n", "u.obj")
    assert np.array_equal(m.corner_normals(), np.zeros((1, 3, 3), F)) and m.corner_uvs() is None   # vn lines: the mesh has normals
    m = same_as_stripped(vx, tmp_path, QUAD + "vt 1 1\nvn 0 0 1\nf 1/0/0 2/5/3 3/-7/-9\nf 1/x/1 2/1/ 3//1\n", "r.obj")
    n, uv = m.corner_normals(), m.corner_uvs()
    assert np.array_equal(n[0], np.zeros((3, 3), F)) and np.array_equal(uv[0], np.zeros((3, 2), F))
    # 1/x/1: no vt, and the vn field is not reached; 2/1/: vt 1, an empty vn
    assert np.array_equal(n[1], F([[0, 0, 0], [0, 0, 0], [0, 0, 1]])) and np.array_equal(uv[1], F([[0, 0], [1, 0], [0, 0]]))
    m = same_as_stripped(vx, tmp_path, QUAD + "f 1/1/1 2/2/2 3/3/3\n", "n.obj")
    assert m.corner_normals() is None and m.corner_uvs() is None    # no vt / vn lines at all


def test_errors_unchanged(vx, tmp_path):
    for k, text in enumerate([QUAD + "vt 0 0\nf 1/1 2/1 9/1\n", QUAD + "vn 0 0 1\nf 0//1 2//1 3//1\n", QUAD + "f 1/1/1 x 3\n",
                              QUAD + "vt 0 0\nf -9/1 2/1 3/1\n", "vt 0 0\nf 1/1 2/1 3/1\nv 0 0 0\nv 1 0 0\nv 0 1 0\n"]):
        same_as_stripped(vx, tmp_path, text, "e%d.obj" % k)


def write_mtl_scene(tmp_path):
    (tmp_path / "tex").mkdir(exist_ok=True)
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 1 1 1\nmap_Kd -s 2 2 1 -o 0.5 0 0 tex/a.ppm\nnewmtl b\nKd 1 0 0\n"
                                    "newmtl c\nmap_Kd c.tga\nnewmtl d\nmap_Kd /nonexistent/d.ppm\n")
    text = "mtllib m.mtl\n" + QUAD + "vt 0 0\nusemtl a\nf 1/1 2/1 3/1\nusemtl c\nf 1 3 4\n"
    (tmp_path / "s.obj").write_text(text)
    return tmp_path / "s.obj"


def test_map_kd_slots(vx, tmp_path):
    m = vx.Mesh.load_obj(str(write_mtl_scene(tmp_path)))
    names = m.texture_names()
    assert names == [str(tmp_path / "tex" / "a.ppm"), str(tmp_path / "c.tga"), "/nonexistent/d.ppm"]
    assert m.material_textures().tolist() == [0, -1, 1, 2]
    recs, _ = m.materials()
    assert (recs["texture_id"] == -1).all()                          # the voxel path's records are unchanged
    assert m.texture(0) is None                                       # loading the OBJ reads no image


def ppm(w, h, px):
    return b"P6\n# comment\n%d %d\n255\n" % (w, h) + np.asarray(px, np.uint8).tobytes()


def tga(w, h, px_top_first, bpp, top, rle=False):
    """px [h, w, 4] RGBA top row first -> TGA bytes (BGR(A), bottom-left origin unless top)"""
    a = np.asarray(px_top_first, np.uint8)
    rows = a if top else a[::-1]
    c = rows[..., [2, 1, 0, 3]] if bpp == 32 else rows[..., [2, 1, 0]]
    flat = c.reshape(-1, bpp // 8)
    if rle:   # one raw packet per pixel pair / a run packet where two neighbours are equal
        body, i = b"", 0
        while i < len(flat):
            if i + 1 < len(flat) and (flat[i] == flat[i + 1]).all():
                body += bytes([0x81]) + flat[i].tobytes()
            else:
                body += bytes([0x00]) + flat[i].tobytes()
                if i + 1 < len(flat):
                    body += bytes([0x00]) + flat[i + 1].tobytes()
            i += 2
    else:
        body = flat.tobytes()
    hdr = struct.pack("<BBBHHBHHHHBB", 0, 0, 10 if rle else 2, 0, 0, 0, 0, 0, w, h, bpp, (0x20 if top else 0) | (8 if bpp == 32 else 0))
    return hdr + body


def test_decoding(vx, tmp_path):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    files = {"p.ppm": ppm(7, 5, img[..., :3])}
    for bpp in (24, 32):
        for top in (False, True):
            for rle in (False, True):
                files["t%d%d%d.tga" % (bpp, top, rle)] = tga(7, 5, img, bpp, top, rle)
    files["trunc.ppm"] = ppm(7, 5, img[..., :3])[:-4]
    files["trunc.tga"] = tga(7, 5, img, 32, True)[:-3]
    files["x.png"] = b"\x89PNG\r\n\x1a\n" + bytes(64)
    files["max.ppm"] = b"P6 7 5 65535\n" + bytes(7 * 5 * 6)
    names = sorted(files) + ["missing.ppm"]
    for k, v in files.items():
        (tmp_path / k).write_bytes(v)
    mtl = "".join("newmtl m%d\nmap_Kd %s\n" % (i, n) for i, n in enumerate(names))
    (tmp_path / "d.mtl").write_text(mtl)
    (tmp_path / "d.obj").write_text("mtllib d.mtl\n" + QUAD + "f 1 2 3\n")
    m = vx.Mesh.load_obj(str(tmp_path / "d.obj"))
    m.load_textures()
    magenta = np.array([[[255, 0, 255, 255]]], np.uint8)
    for i, n in enumerate(names):
        got = m.texture(i)
        if n.startswith("t") and n.endswith(".tga") and n != "trunc.tga":
            want = img.copy() if n[1:3] == "32" else np.concatenate([img[..., :3], np.full((5, 7, 1), 255, np.uint8)], 2)
            assert np.array_equal(got, want), n
        elif n == "p.ppm":
            assert np.array_equal(got[..., :3], img[..., :3]) and (got[..., 3] == 255).all()
        else:
            assert np.array_equal(got, magenta), n


def test_argument_errors(vx):
    m = vx.Mesh.from_arrays(F([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[0, 1, 2]]))
    for w, h in [(0, 1), (1, 0), (16385, 1), (1, 16385)]:
        with pytest.raises(vx.VxError) as e:
            vx._check(vx.lib().vx_mesh_set_texture(m.h, 0, w, h, np.zeros(16, np.uint8).ctypes.data))
        assert e.value.status == 1                              # VX_ERR_INVALID_ARG
    with pytest.raises(vx.VxError):
        m.set_texture(-1, np.zeros((1, 1, 4), np.uint8))
    with pytest.raises(vx.VxError):
        m.set_material_textures([0])                                   # the mesh has no materials
    assert vx.lib().vx_render_set_shading(None, vx.RENDER_ATTRIBUTES) == 1
    assert vx.lib().vx_mesh_set_attributes(None, None, None) == 1
    assert vx.lib().vx_mesh_load_textures(None) == 1
    m.set_texture(3, np.full((2, 3, 3), 7, np.uint8))
    assert m.texture_names() == ["", "", "", ""] and m.texture(0) is None and m.texture(3).shape == (2, 3, 4)
    nrm = np.arange(9, dtype=F).reshape(1, 3, 3)
    m.set_attributes(normals=nrm)
    assert np.array_equal(m.corner_normals(), nrm) and m.corner_uvs() is None
    m.set_attributes(uvs=np.ones((1, 3, 2), F))
    assert m.corner_normals() is None and np.array_equal(m.corner_uvs(), np.ones((1, 3, 2), F))


# ---- hand-worked cases of attr_ref -----------------------------------------------------------------------------------------------
def test_bilinear_at_texel_centres():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    y, x = np.mgrid[0:3, 0:5]
    uv = np.stack([(x.ravel() + F(0.5)) / F(5), (y.ravel() + F(0.5)) / F(3)], 1).astype(F)
    got = attr_ref.sample(img, uv)
    assert np.array_equal(got, attr_ref.SRGB[img[y.ravel(), x.ravel(), :3]])


def test_wrap_around():
    img = np.zeros((1, 4, 4), np.uint8)
    img[0, :, 0] = [0, 255, 0, 255]
    assert attr_ref.tex_axis(F([0.0]), 4)[:2] == (3, 0)                 # x = -0.5: texels 3 and 0, weight 0.5
    assert attr_ref.tex_axis(F([1.0]), 4)[:2] == (3, 0)                 # x = 3.5
    i0, i1, f = attr_ref.tex_axis(F([-0.375]), 4)                      # x = -2: texel 2 and 3, weight 0
    assert (i0, i1, f[0]) == (2, 3, 0)
    s = attr_ref.sample(img, F([[0.0, 0.5], [1.0, 0.5], [-0.75 + 0.125, 0.5], [1.25 + 0.125, 0.5]]))
    assert np.array_equal(s[:, 0], F([0.5, 0.5, 1.0, 1.0])) and not s[:, 1:].any()


def test_srgb_table_endpoints():
    t = attr_ref.SRGB
    assert t.dtype == np.float32 and t[0] == 0 and t[255] == 1
    assert t[10] == F(10 / 255 / 12.92) and t[11] == F(((11 / 255 + 0.055) / 1.055) ** 2.4)   # 10/255 <= 0.04045 < 11/255
    assert (np.diff(t) > 0).all()


def test_non_finite_uv():
    for u in (np.nan, np.inf, -np.inf, 2.0 ** 62, -(2.0 ** 63)):
        i0, i1, f = attr_ref.tex_axis(F([u]), 7)
        assert (i0[0], i1[0], f[0]) == (0, 0, 0), u
    i0, i1, f = attr_ref.tex_axis(F([3.0 * 2.0 ** 38]), 7)              # beyond 32 bits: x = 21 * 2^38 exactly, a multiple of 7
    assert (i0[0], i1[0], f[0]) == (0, 1, 0)
    i0, i1, f = attr_ref.tex_axis(F([-(2.0 ** 36)]), 5)                  # -5 * 2^36: residue 0, non-negative
    assert (i0[0], i1[0], f[0]) == (0, 1, 0)
    img = np.zeros((2, 2, 4), np.uint8)
    img[0, 0, :3] = 255
    assert np.array_equal(attr_ref.sample(img, F([[np.nan, np.inf]])), F([[1, 1, 1]]))


def test_texture_after_ambient():
    d = F([[0, 0, -1]])
    kind = np.uint8([2])
    N = F([[0, 0, 1]])
    L = F([[0, 0, 1]])
    mmat = render_ref.per_pixel_materials(None, None, 1)
    mmat["illum"][:] = 1
    mmat["diffuse"][:] = F([0.5, 0.5, 0.5])
    mmat["ambient"][:] = F([0.25, 0.25, 0.25])
    light = (F([0, 0, 1]), F(1), 1)
    rgba, _ = attr_ref.shade(d, kind, np.zeros((1, 3), F), N, L, np.full(1, 1e5, F), [0], [0], light, None, mmat, F([[0.5, 1.0, 0.0]]))
    c = F([0.375, 0.75, 0.0])                       # (0.5*1 + 0.25) * tex
    want = np.floor(np.power(c, F(1) / F(2.2)) * F(255) + F(0.5)).astype(np.uint8)
    assert np.array_equal(rgba[0, :3], want)


def test_normal_fallback_and_world():
    n = attr_ref.unit(F([[0, 0, 0], [3, 0, 4], [np.inf, 0, 0]]), F([[9, 9, 9]] * 3))
    assert np.array_equal(n, F([[9, 9, 9], [0.6, 0, 0.8], [9, 9, 9]]))
    w = np.zeros((1, 12), F)
    w[0, [0, 5, 10]] = F(2)
    w[0, 1] = F(1)                                  # W = [[2, 1, 0], [0, 2, 0], [0, 0, 2]]: W^T n
    assert np.array_equal(attr_ref.world_normals(F([[1, 1, 1]]), w), F([[2, 3, 2]]))
