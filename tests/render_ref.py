"""numpy restatement of a device frame's per-pixel stages (vx_render_frame_device, csrc/vx_render.hip) in float32: the shadow ray of every
pixel from the merged primary hits, and the shading of raytrace2.rchit (voxels) / raytrace.rchit (triangles) with the miss colour and the
gamma -- cpp/voxilizer.cpp render()'s arithmetic, generalised to the light of vx_render_light.  It takes the traversals' outputs as input
(no ray tracing here): t / prim / normal of the voxel hits, t / prim / bary / normal of the triangle hits, and the two shadow flags."""
import numpy as np

F = np.float32
DEFAULT_LIGHT = (F([10.0, 55.0, 8.0]), F(1000.0), 0)          # hello_vulkan.h:84-90: point light
MISS = F(0.8)                                                # rmiss:37
DEFAULT_MAT = dict(ambient=F([0.1, 0.1, 0.1]), diffuse=F([1, 1, 0]), specular=F([1, 1, 1]), shininess=F(0), illum=0)   # MaterialObj{}


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def host_dirs(vi, pi, W, H):
    """render()'s primary directions: tg = norm(((pi0*dx + pi4*dy) + pi8) + pi12 ...) dividing by the length, dir = viewInv * tg"""
    vi, pi = F(vi).reshape(16), F(pi).reshape(16)
    i = np.arange(W * H)
    u = ((i % W).astype(F) + F(0.5)) / F(W)
    v = ((i // W).astype(F) + F(0.5)) / F(H)
    dx, dy = u * F(2) - F(1), v * F(2) - F(1)
    tg = np.stack([((pi[k] * dx + pi[4 + k] * dy) + pi[8 + k]) + pi[12 + k] for k in range(3)], 1)
    tg = tg / np.sqrt(_dot(tg, tg))[:, None]
    return np.stack([(vi[k] * tg[:, 0] + vi[4 + k] * tg[:, 1]) + vi[8 + k] * tg[:, 2] for k in range(3)], 1)


def merge(vt, mt):
    """-> kind per pixel: 0 miss, 1 voxel, 2 triangle (the closer hit; the voxel on equal t)"""
    vt = F(vt)
    tri = np.zeros(vt.shape, bool) if mt is None else (F(mt) > 0) & ~((vt > 0) & (vt <= F(mt)))
    return np.where(tri, 2, np.where(vt > 0, 1, 0)).astype(np.uint8)


def shadow_rays(org, d, kind, vt, mt=None, mprim=None, mbary=None, verts=None, tris=None, light=DEFAULT_LIGHT):
    """-> (rays [n, 6] = hit point + L, dist [n] = the shadow ray's tMax); light = (position, intensity, type 0 point / 1 directional)"""
    pos_l, _, ltype = light
    pos_l = F(pos_l)
    tri = kind == 2
    ts = np.where(tri, F(mt) if mt is not None else F(0), np.where(F(vt) > 0, F(vt), F(0)))
    wp = F(org)[None, :] + d * ts[:, None]
    if ltype == 1:                                           # rchit:86-91: L = normalize(lightPosition), distance 100000
        l = np.broadcast_to(pos_l, wp.shape).astype(F)
    else:
        pos = wp.copy()
        k = np.flatnonzero(tri)
        if k.size:
            tv = F(verts)[np.asarray(tris)[mprim[k].astype(np.int64)]]      # [m, 3, 3]
            b1, b2 = F(mbary)[k, 0], F(mbary)[k, 1]
            b0 = (F(1) - b1) - b2
            pos[k] = (tv[:, 0] * b0[:, None] + tv[:, 1] * b1[:, None]) + tv[:, 2] * b2[:, None]   # rchit:67-68
        l = pos_l[None, :] - pos
    length = np.sqrt(_dot(l, l))
    L = l * (F(1) / length)[:, None]
    dist = np.full(length.shape, F(100000), F) if ltype == 1 else length
    return np.ascontiguousarray(np.concatenate([wp, L], 1).astype(F)), dist


def per_pixel_materials(table, ids, n):
    """material fields per pixel from a MATERIAL table and per-pixel indices (out of range / negative / no table: MaterialObj{})"""
    out = dict(ambient=np.tile(DEFAULT_MAT["ambient"], (n, 1)), diffuse=np.tile(DEFAULT_MAT["diffuse"], (n, 1)),
               specular=np.tile(DEFAULT_MAT["specular"], (n, 1)), shininess=np.full(n, DEFAULT_MAT["shininess"], F), illum=np.zeros(n, np.int64))
    if table is None or ids is None or len(table) == 0:
        return out
    ids = np.asarray(ids, np.int64)
    ok = (ids >= 0) & (ids < len(table))
    rec = table[ids[ok]]
    for f in ("ambient", "diffuse", "specular"):
        out[f][ok] = F(rec[f])
    out["shininess"][ok] = F(rec["shininess"])
    out["illum"][ok] = rec["illum"]
    return out


def shade(d, kind, vnormal, mnormal, L, dist, sv, sm, light=DEFAULT_LIGHT, vmat=None, mmat=None):
    """-> (rgba uint8 [n, 4], shadowed uint8 [n]: the OR of the two shadow flags where the shading reads it, 0 elsewhere).
    vmat / mmat: per_pixel_materials of the voxel / triangle hits (None: MaterialObj{} everywhere)."""
    n = len(kind)
    _, intensity, ltype = light
    vmat = vmat or per_pixel_materials(None, None, n)
    mmat = mmat or per_pixel_materials(None, None, n)
    tri, vox = kind == 2, kind == 1
    N = np.where(tri[:, None], F(mnormal) if mnormal is not None else F(0), F(vnormal)).astype(F)
    flip = tri & (_dot(N, d) > 0)
    N[flip] = N[flip] * F(-1)                                           # the geometric normal, toward the ray
    mat = {k: np.where(tri[:, None] if vmat[k].ndim == 2 else tri, mmat[k], vmat[k]) for k in vmat}
    li = np.full(n, F(intensity), F) if ltype == 1 else F(intensity) / (dist * dist)   # rchit:83 / :85
    dnl0 = _dot(N, L)
    dnl = np.fmax(dnl0, F(0))                                           # computeDiffuse, wavefront.glsl:25
    diff = mat["diffuse"] * dnl[:, None]
    diff = np.where((mat["illum"] >= 1)[:, None], diff + mat["ambient"], diff)
    lit = dnl0 > 0
    sh = lit & ((np.asarray(sv) != 0) | (np.asarray(sm) != 0 if sm is not None else False))
    att = np.where(lit, np.where(sh, F(0.3), F(1)), np.where(tri, F(1), F(0.3))).astype(F)
    spec = np.zeros_like(diff)
    s = lit & ~sh & (mat["illum"] >= 2) & (kind > 0)
    if s.any():                                                          # computeSpecular, wavefront.glsl:32-48
        kSh = np.fmax(mat["shininess"][s], F(4))
        kE = (F(2) + kSh) / (F(2) * F(3.14159265))
        e = d[s] * F(-1)
        V = e / np.sqrt(_dot(e, e))[:, None]
        I = L[s] * F(-1)
        Rr = I - N[s] * (F(2) * _dot(N[s], I))[:, None]
        sp = kE * np.power(np.fmax(_dot(V, Rr), F(0)), kSh)
        spec[s] = mat["specular"][s] * sp[:, None]
    c = (li * att)[:, None] * (diff + spec)
    c[kind == 0] = MISS
    g = np.power(np.fmin(np.fmax(c, F(0)), F(1)), F(1.0) / F(2.2))    # post.frag:36; fmaxf / fminf: a NaN channel is 0, so g is in [0, 1]
    rgb = np.floor(np.nan_to_num(g, nan=0.0) * F(255) + F(0.5)).astype(np.uint8)
    rgba = np.concatenate([rgb, np.full((n, 1), 255, np.uint8)], 1)
    return rgba, (sh & (kind > 0)).astype(np.uint8)
