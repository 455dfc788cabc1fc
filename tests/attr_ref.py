"""numpy float32 restatement of attribute shading (vx_render_set_shading(VX_RENDER_ATTRIBUTES), include/voxhip.h): the normal of a triangle hit
from its corner normals or its face, moved to world space by W^T, the bilinear sRGB texture of its material, and the shading of render_ref
with that normal (not turned toward the ray) and diffuse *= tex after the ambient term.  Like render_ref it takes the traversals' outputs as
input (t, prim, bary, instance, the geometric normal, the shadow flags) and Tlas.world_to_object() for instances; render_ref's helpers give
the directions, the merge, the shadow rays and the material records."""
import numpy as np

import render_ref

F = np.float32
TWO62 = F(2.0 ** 62)


def srgb_table():
    """the sRGB EOTF of c / 255 for every byte c, in float64, rounded to float32"""
    x = np.arange(256, dtype=np.float64) / 255.0
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4).astype(F)


SRGB = srgb_table()


def bary3(b):
    b = F(b).reshape(-1, 2)
    b1, b2 = b[:, 0], b[:, 1]
    return (F(1) - b1) - b2, b1, b2


def interp(c, b0, b1, b2):
    """(c0*b0 + c1*b1) + c2*b2 over corners c [m, 3, k]"""
    return (c[:, 0] * b0[:, None] + c[:, 1] * b1[:, None]) + c[:, 2] * b2[:, None]


def object_normals(verts, tris, cnrm, prim, bary):
    """[m, 3]: the corner normals interpolated, or (cnrm None) the face normal cross(p1 - p0, p2 - p0), unnormalised"""
    prim = np.asarray(prim, np.int64)
    b0, b1, b2 = bary3(bary)
    if cnrm is not None:
        return interp(F(cnrm).reshape(-1, 3, 3)[prim], b0, b1, b2)
    p = F(verts).reshape(-1, 3)[np.asarray(tris).reshape(-1, 3)[prim]]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F)


def world_normals(n, w2o=None):
    """W^T n per row, W the row-major world-to-object 3x3 (w2o [m, 12]; None: n itself), component j = (w0j*n0 + w1j*n1) + w2j*n2"""
    n = F(n)
    if w2o is None:
        return n
    w = F(w2o).reshape(-1, 12)
    return np.stack([(w[:, j] * n[:, 0] + w[:, 4 + j] * n[:, 1]) + w[:, 8 + j] * n[:, 2] for j in range(3)], 1).astype(F)


def unit(n, fallback):
    """n / sqrtf(dot(n, n)); where that is zero or not finite: fallback (the default normal)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        N = n / np.sqrt(render_ref._dot(n, n))[:, None]
    ok = np.isfinite(N).all(1) & (N != 0).any(1)
    return np.where(ok[:, None], N, F(fallback)).astype(F)


def toward_ray(g, d):
    """the default normal of a triangle hit: the geometric normal turned toward the ray"""
    g = F(g).copy()
    flip = render_ref._dot(g, F(d)) > 0
    g[flip] = g[flip] * F(-1)
    return g


def tex_axis(u, w):
    """x = u*w - 0.5: (i0 = floor(x) mod w non-negative, i1 = (i0 + 1) mod w, f = x - floor(x)); non-finite or |x| >= 2^62: (0, 0, 0)"""
    with np.errstate(invalid="ignore", over="ignore"):
        x = F(u) * F(w) - F(0.5)
        ok = np.abs(x) < TWO62
        fl = np.floor(np.where(ok, x, F(0)))
        f = np.where(ok, x - fl, F(0)).astype(F)
    i0 = np.where(ok, np.mod(fl.astype(np.int64), w), 0)
    return i0, np.where(ok, (i0 + 1) % w, 0), f


def sample(img, uv):
    """bilinear rgb of an RGBA8 image [h, w, 4] (top row first) at uv [m, 2], texels decoded by SRGB, float weights, repeat addressing"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    uv = F(uv).reshape(-1, 2)
    x0, x1, fx = tex_axis(uv[:, 0], w)
    y0, y1, fy = tex_axis(uv[:, 1], h)
    lin = SRGB[img[..., :3]]
    gx, gy = (F(1) - fx)[:, None], (F(1) - fy)[:, None]
    fx, fy = fx[:, None], fy[:, None]
    return ((lin[y0, x0] * gx + lin[y0, x1] * fx) * gy + (lin[y1, x0] * gx + lin[y1, x1] * fx) * fy).astype(F)


MAGENTA = np.array([[[255, 0, 255, 255]]], np.uint8)


def texture_factor(prim, bary, mat_ids, slots, images, cuv):
    """[m, 3] multiplier of the diffuse term (1 where the triangle's material has no texture slot that exists).  mat_ids: per triangle (None:
    no materials), slots: per material, images: per slot (None: the 1x1 magenta of a slot without an image), cuv [T, 3, 2] or None"""
    m = len(prim)
    out = np.ones((m, 3), F)
    if mat_ids is None or slots is None or len(slots) == 0:
        return out
    prim = np.asarray(prim, np.int64)
    mi = np.asarray(mat_ids, np.int64)[prim]
    ok = (mi >= 0) & (mi < len(slots))
    sl = np.where(ok, np.asarray(slots, np.int64)[np.clip(mi, 0, len(slots) - 1)], -1)
    b0, b1, b2 = bary3(bary)
    c = F(cuv).reshape(-1, 3, 2)[prim] if cuv is not None else np.zeros((m, 3, 2), F)
    uv = interp(c, b0, b1, b2)
    for s in range(len(images)):
        k = sl == s
        if k.any():
            out[k] = sample(images[s] if images[s] is not None else MAGENTA, uv[k])
    return out


def shade(d, kind, vnormal, tnormal, L, dist, sv, sm, light=render_ref.DEFAULT_LIGHT, vmat=None, mmat=None, tex=None):
    """render_ref.shade with tnormal (the final N of triangle hits, not turned) and tex ([n, 3] diffuse multiplier of triangle hits, None: 1)"""
    n = len(kind)
    _, intensity, ltype = light
    vmat = vmat or render_ref.per_pixel_materials(None, None, n)
    mmat = mmat or render_ref.per_pixel_materials(None, None, n)
    tri = kind == 2
    N = np.where(tri[:, None], F(tnormal), F(vnormal)).astype(F)
    mat = {k: np.where(tri[:, None] if vmat[k].ndim == 2 else tri, mmat[k], vmat[k]) for k in vmat}
    li = np.full(n, F(intensity), F) if ltype == 1 else F(intensity) / (dist * dist)
    dnl0 = render_ref._dot(N, L)
    dnl = np.fmax(dnl0, F(0))
    diff = mat["diffuse"] * dnl[:, None]
    diff = np.where((mat["illum"] >= 1)[:, None], diff + mat["ambient"], diff)
    if tex is not None:
        diff = np.where(tri[:, None], diff * F(tex), diff).astype(F)     # after the ambient term (rchit:99-104)
    lit = dnl0 > 0
    sh = lit & ((np.asarray(sv) != 0) | (np.asarray(sm) != 0 if sm is not None else False))
    att = np.where(lit, np.where(sh, F(0.3), F(1)), np.where(tri, F(1), F(0.3))).astype(F)
    spec = np.zeros_like(diff)
    s = lit & ~sh & (mat["illum"] >= 2) & (kind > 0)
    if s.any():
        kSh = np.fmax(mat["shininess"][s], F(4))
        kE = (F(2) + kSh) / (F(2) * F(3.14159265))
        e = d[s] * F(-1)
        V = e / np.sqrt(render_ref._dot(e, e))[:, None]
        I = L[s] * F(-1)
        Rr = I - N[s] * (F(2) * render_ref._dot(N[s], I))[:, None]
        sp = kE * np.power(np.fmax(render_ref._dot(V, Rr), F(0)), kSh)
        spec[s] = mat["specular"][s] * sp[:, None]
    c = (li * att)[:, None] * (diff + spec)
    c[kind == 0] = render_ref.MISS
    g = np.power(np.fmin(np.fmax(c, F(0)), F(1)), F(1.0) / F(2.2))       # fmaxf / fminf: a NaN channel is 0, so g is in [0, 1]
    rgb = np.floor(np.nan_to_num(g, nan=0.0) * F(255) + F(0.5)).astype(np.uint8)
    rgba = np.concatenate([rgb, np.full((n, 1), 255, np.uint8)], 1)
    return rgba, (sh & (kind > 0)).astype(np.uint8)


class MeshAttr:
    """what the shading reads of one mesh: verts, tris, corner normals / uvs (None: none), material table and per-triangle ids (None: none),
    per-material slots and per-slot images"""

    def __init__(self, verts, tris, cnrm=None, cuv=None, mats=None, ids=None, slots=None, images=()):
        self.verts, self.tris, self.cnrm, self.cuv = verts, tris, cnrm, cuv
        self.mats, self.ids, self.slots, self.images = mats, ids, slots, list(images)

    @classmethod
    def of(cls, mesh):
        """from a voxhip.Mesh"""
        v, t = mesh.host_arrays()
        mats, ids = mesh.materials()
        nt = mesh.num_triangles
        images = [mesh.texture(k) for k in range(len(mesh.texture_names()))]
        return cls(v, t, mesh.corner_normals(), mesh.corner_uvs(), mats if len(mats) else None, ids, mesh.material_textures(), images)


def tri_pixels(d, k, meshes, which, prim, bary, gnormal, w2o=None):
    """(N [m, 3], tex [m, 3], mats dict) of triangle pixels k: meshes[which[k]]"""
    m = len(k)
    N = np.zeros((m, 3), F)
    T = np.ones((m, 3), F)
    ids = np.full(m, -1, np.int64)
    tabs = {}
    for b in np.unique(which):
        sel = which == b
        ma = meshes[int(b)]
        pr, ba = prim[k[sel]], bary[k[sel]]
        n = world_normals(object_normals(ma.verts, ma.tris, ma.cnrm, pr, ba), None if w2o is None else w2o[sel])
        N[sel] = unit(n, toward_ray(gnormal[k[sel]], d[k[sel]]))
        T[sel] = texture_factor(pr, ba, ma.ids, ma.slots, ma.images, ma.cuv)
        if ma.ids is not None:
            ids[sel] = np.asarray(ma.ids, np.int64)[np.asarray(pr, np.int64)]
        tabs[int(b)] = sel
    return N, T, ids, tabs


def frame(cam, vo, mo, meshes, sv, sm, rays, dist, light=render_ref.DEFAULT_LIGHT, inst=None, w2o=None):
    """the attribute frame from the traversals: vo = voxel trace (t, normal) or None, mo = triangle trace (t, prim, bary, normal and, for
    instances, instance), meshes = [MeshAttr] (one per BLAS; [0] in a BVH scene), inst = the instance records (blas), w2o = world_to_object()
    -> dict(rgba, kind, shadowed)"""
    vi, pi, W, H = cam
    n = W * H
    d = render_ref.host_dirs(vi, pi, W, H)
    vt = vo["t"] if vo is not None else np.full(n, -1, F)
    vn = vo["normal"] if vo is not None else np.zeros((n, 3), F)
    kind = render_ref.merge(vt, mo["t"])
    k = np.flatnonzero(kind == 2)
    if inst is not None:
        ii = mo["instance"][k].astype(np.int64)
        which = np.asarray(inst["blas"], np.int64)[ii]
        wk = F(w2o).reshape(-1, 12)[ii]
    else:
        which = np.zeros(len(k), np.int64)
        wk = None
    N, T, ids, tabs = tri_pixels(d, k, meshes, which, mo["prim"], F(mo["bary"]), F(mo["normal"]), wk)
    tn = np.zeros((n, 3), F)
    tn[k] = N
    tex = np.ones((n, 3), F)
    tex[k] = T
    mmat = render_ref.per_pixel_materials(None, None, n)
    for b, sel in tabs.items():
        ma = meshes[b]
        if ma.mats is None:
            continue
        pm = render_ref.per_pixel_materials(ma.mats, ids[sel], int(sel.sum()))
        for f in mmat:
            mmat[f][k[sel]] = pm[f]
    rgba, sh = shade(d, kind, vn, tn, rays[:, 3:], dist, sv, sm, light, None, mmat, tex)
    return dict(rgba=rgba, kind=kind, shadowed=sh)
