"""Probe sheets, cases and the high-precision comparison for the frame shaders (csrc/vx_render.hip) at the material, light, normal and
texture values the ordinary pictures never reach.  A helper for tests/test_shading_extremes_cpu.py and tests/test_gpu_shading_extremes.py,
not a test itself (the rules under test: include/voxhip.h, "shading at its extremes").

A probe sheet is a planar grid of Q x R quads at z = 0 (two triangles each, vertices not shared) seen head-on by a camera on the -z axis, so
that every quad covers px x px pixels and carries its own material, uvs and corner normals: one frame is a table of cases.

prepare() / expected() take what attr_ref.frame and test_gpu_render.reference take -- the traversals' outputs -- and evaluate every stage in
float32 exactly as render_ref / attr_ref do, except the two powf calls: those are computed in float64 from their float32 arguments (the
specular one is then rounded to float32; the gamma is kept as y = 255 * c^(1/2.2) in float64).  compare() then asks for the byte
floor(y + 0.5) EXACTLY wherever y is at least M_TIE away from a rounding tie, and within 1 elsewhere.

Sheets and their brute-force traversals are cached per process and read-only."""
import functools
import types

import numpy as np

import attr_ref
import instance_ref
import mesh_ref
import render_ref

F = np.float32
FLT_MAX = np.finfo(F).max
SUBNORMAL = F(1e-45)                                  # the smallest positive float32, 2^-149
INT32_MIN = -2 ** 31
MATERIAL = np.dtype([("ambient", F, 3), ("diffuse", F, 3), ("specular", F, 3), ("transmittance", F, 3), ("emission", F, 3), ("shininess", F),
                     ("ior", F), ("dissolve", F), ("illum", np.int32), ("texture_id", np.int32)])      # voxhip.MATERIAL
GAMMA_EXP = float(F(1.0) / F(2.2))                    # the float32 exponent of the kernel's powf, as a float64
# The margin around a rounding tie inside which a byte may differ by 1: 8 x the largest distance from a tie at which the device's byte was
# seen to differ from floor(y + 0.5) over every frame of this module (measured: it never differs, 0), and no less than 2^-12.
M_TIE = 2.0 ** -12
M_TIE_MAX = 2.0 ** -7                                 # a larger measured margin is a finding, not a tolerance
NEAR_SHARE_MAX = 0.03                                 # at most 3 % of a frame's hit-pixel channels within M_TIE of a tie (uniform: 2 m)
DISTINCT_MIN = 32                                     # distinct byte values among a frame's hit pixels, unless the case says why it is flat
MISS_RGBA = (230, 230, 230, 255)


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def material(ambient=0.1, diffuse=0.7, specular=0.0, shininess=16.0, illum=1):
    rec = np.zeros(1, MATERIAL)
    rec["ambient"], rec["diffuse"], rec["specular"], rec["shininess"], rec["illum"] = F(ambient), F(diffuse), F(specular), F(shininess), illum
    return rec


def table(recs):
    return np.concatenate(recs) if len(recs) else np.zeros(0, MATERIAL)


# ---- the probe sheet ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sheet(Q, R, px=8, x0=0.0, z=0.0, total_q=None):
    """Q x R unit quads at depth z, wound so that the face normal is -z (toward the camera).  Quad q = j*Q + i has the triangles 2q, 2q + 1
    and the corners a (0, 0), c (1, 1), b (1, 0) / a, d (0, 1), c; `corner` gives the (s, t) of every triangle corner in the quad's unit
    square.  The camera frames total_q x R quads (default Q) centred on x = 0; x0 shifts this sheet inside that frame."""
    TQ = total_q or Q
    W, H = TQ * px, R * px
    i, j = np.meshgrid(np.arange(Q), np.arange(R))
    ox, oy = (i.ravel() - Q / 2.0 + x0), (j.ravel() - R / 2.0)
    st = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)                       # a b c d
    verts = np.zeros((Q * R, 4, 3))
    verts[:, :, 0] = ox[:, None] + st[None, :, 0]
    verts[:, :, 1] = oy[:, None] + st[None, :, 1]
    verts[:, :, 2] = z
    base = 4 * np.arange(Q * R)[:, None]
    tris = np.stack([base + [0, 2, 1], base + [0, 3, 2]], 1).reshape(-1, 3)
    corner = np.tile(np.stack([st[[0, 2, 1]], st[[0, 3, 2]]]), (Q * R, 1, 1))          # [T, 3, 2]
    import vx_scenes
    D = (R / 2.0) / np.tan(np.radians(30.0))                                          # the frame is exactly R quads high at z = 0
    vi, pi = vx_scenes.camera_matrices(eye=(0.0, 0.0, -D), ctr=(0.0, 0.0, 0.0), aspect=W / H)
    return _ns(Q=Q, R=R, px=px, W=W, H=H, n=W * H, nq=Q * R, nt=2 * Q * R, verts=_frozen(verts.reshape(-1, 3).astype(F)),
               tris=_frozen(tris.astype(np.int32)), corner=_frozen(corner.astype(F)), cam=(_frozen(vi), _frozen(pi), W, H), D=D)


def quad_of(prim):
    return np.asarray(prim, np.int64) // 2


def per_quad(vals):
    """[nq, ...] -> [T, 3, ...]: the same value on the three corners of both triangles of a quad"""
    v = np.asarray(vals)
    return np.repeat(np.repeat(v[:, None], 2, 0).reshape((-1,) + v.shape[1:])[:, None], 3, 1)


@functools.lru_cache(maxsize=None)
def cpu_trace(Q, R, px=8):
    """mesh_ref's brute force of the sheet's camera rays: what the GPU tests take from Bvh.trace_ex (the sheet is planar, so this is cheap)"""
    sh = sheet(Q, R, px)
    vi, pi, W, H = sh.cam
    d = render_ref.host_dirs(vi, pi, W, H)
    rays = np.concatenate([np.tile(F(vi[12:15]), (W * H, 1)), d], 1)
    t, prim, bary = mesh_ref.closest(sh.verts, sh.tris, rays)
    return dict(t=_frozen(t), prim=_frozen(prim), bary=_frozen(bary), normal=_frozen(mesh_ref.normals(sh.verts, sh.tris, prim)))


def spec_mesh(verts, tris, cnrm=None, cuv=None, mats=None, ids=None, slots=None, images=()):
    """what a voxhip.Mesh is built from, and what attr_ref.MeshAttr holds; images[s] None: a slot without an image (magenta)"""
    return attr_ref.MeshAttr(verts, tris, cnrm, cuv, mats, ids, slots, images)


def build_mesh(vx, ma):
    m = vx.Mesh.from_arrays(ma.verts, ma.tris)
    if ma.cnrm is not None or ma.cuv is not None:
        m.set_attributes(ma.cnrm, ma.cuv)
    if ma.mats is not None:
        m.set_materials(ma.mats, ma.ids)
        if ma.slots is not None:
            m.set_material_textures(ma.slots)
    for s, img in enumerate(ma.images):
        if img is not None:
            m.set_texture(s, img)
    return m


# ---- the high-precision evaluation ------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return render_ref._dot(a, b)


def prepare(cam, vo, mo, meshes, light, attributes, vox_materials=None, inst=None, w2o=None):
    """everything before the shadow query, in float32 as the restatements have it.  vo: the voxel trace (t, prim, normal) or None; mo: the
    triangle trace (t, prim, bary, normal and, with inst, instance); meshes: [MeshAttr] per BLAS; vox_materials: (table, per-voxel ids).
    -> namespace with kind, the shading normal N, the shadow rays, dist, `lit` and tmax (dist where dot(N, L) > 0, else 0: the empty
    interval), the material fields and the texture factor per pixel"""
    vi, pi, W, H = cam
    n = W * H
    with np.errstate(all="ignore"):
        d = render_ref.host_dirs(vi, pi, W, H)
        vt = F(vo["t"]) if vo is not None else np.full(n, -1, F)
        vn = F(vo["normal"]) if vo is not None else np.zeros((n, 3), F)
        kind = render_ref.merge(vt, mo["t"])
        k = np.flatnonzero(kind == 2)
        prim, bary = np.asarray(mo["prim"]), F(mo["bary"]).reshape(-1, 2)
        if inst is not None:
            ii = np.asarray(mo["instance"])[k].astype(np.int64)
            which = np.asarray(inst["blas"], np.int64)[ii]
            wk = F(w2o).reshape(-1, 12)[ii]
            xf = F(inst["transform"]).reshape(-1, 12)[ii]
        else:
            which, wk, xf = np.zeros(len(k), np.int64), None, None
        # the position the barycentrics interpolate, moved to world space by M in the pinned association
        pos = np.zeros((n, 3), F)
        b0, b1, b2 = attr_ref.bary3(bary[k])
        for b in np.unique(which):
            sel = which == b
            ma = meshes[int(b)]
            p = F(ma.verts).reshape(-1, 3)[np.asarray(ma.tris).reshape(-1, 3)[prim[k[sel]].astype(np.int64)]]
            h = attr_ref.interp(p, b0[sel], b1[sel], b2[sel])
            if xf is not None:
                m = xf[sel]
                h = np.stack([((m[:, 4 * r] * h[:, 0] + m[:, 4 * r + 1] * h[:, 1]) + m[:, 4 * r + 2] * h[:, 2]) + m[:, 4 * r + 3] for r in range(3)], 1)
            pos[k[sel]] = h
        # normals, texture factors and materials of the triangle pixels
        tex = np.ones((n, 3), F)
        N = vn.copy()
        mmat = render_ref.per_pixel_materials(None, None, n)
        fallback = attr_ref.toward_ray(F(mo["normal"])[k], d[k])
        nfall = 0
        if attributes:
            Nk, Tk, ids, tabs = attr_ref.tri_pixels(d, k, meshes, which, prim, bary, F(mo["normal"]), wk)
            N[k], tex[k] = Nk, Tk
            raw = np.zeros((len(k), 3), F)
            for b in np.unique(which):
                sel = which == b
                ma = meshes[int(b)]
                raw[sel] = attr_ref.world_normals(attr_ref.object_normals(ma.verts, ma.tris, ma.cnrm, prim[k[sel]], bary[k[sel]]),
                                                  None if wk is None else wk[sel])
            U = raw / np.sqrt(_dot(raw, raw))[:, None]
            fell = ~(np.isfinite(U).all(1) & (U != 0).any(1))
            nfall = int(fell.sum())
        else:
            N[k] = fallback
            fell = np.zeros(len(k), bool)
            ids = np.full(len(k), -1, np.int64)
            tabs = {}
            for b in np.unique(which):
                sel = which == b
                tabs[int(b)] = sel
                if meshes[int(b)].ids is not None:
                    ids[sel] = np.asarray(meshes[int(b)].ids, np.int64)[prim[k[sel]].astype(np.int64)]
        for b, sel in tabs.items():
            ma = meshes[b]
            if ma.mats is None or len(ma.mats) == 0:
                continue
            pm = render_ref.per_pixel_materials(ma.mats, ids[sel], int(sel.sum()))
            for f in mmat:
                mmat[f][k[sel]] = pm[f]
        vmat = None
        if vox_materials is not None and vo is not None:
            tab, vids = vox_materials
            vp = np.asarray(vo["prim"]).astype(np.int64)
            ok = (vt > 0) & (vp < len(vids))
            pid = np.full(n, -1, np.int64)
            pid[ok] = np.asarray(vids, np.int64)[vp[ok]]
            vmat = render_ref.per_pixel_materials(tab, pid, n)
        vmat = vmat or render_ref.per_pixel_materials(None, None, n)
        tri = kind == 2
        mat = {f: np.where(tri[:, None] if vmat[f].ndim == 2 else tri, mmat[f], vmat[f]) for f in vmat}
        # the shadow ray
        pos_l, _, ltype = light
        pos_l = F(pos_l)
        ts = np.where(tri, F(mo["t"]), np.where(vt > 0, vt, F(0)))
        wp = F(vi[12:15])[None, :] + d * ts[:, None]
        if ltype == 1:
            l = np.broadcast_to(pos_l, wp.shape).astype(F)
        else:
            src = wp.copy()
            src[tri] = pos[tri]
            l = pos_l[None, :] - src
        length = np.sqrt(_dot(l, l))
        L = (l * (F(1) / length)[:, None]).astype(F)
        dist = np.full(n, F(100000), F) if ltype == 1 else length.astype(F)
        dnl0 = _dot(N, L)
        lit = (kind > 0) & (dnl0 > 0)                                                 # false for a NaN dot
    rays = np.ascontiguousarray(np.concatenate([wp, L], 1).astype(F))
    fell_px = np.zeros(n, bool)
    fell_px[k] = fell
    return _ns(cam=cam, n=n, d=d, kind=kind, N=N, L=L, dist=dist, rays=rays, lit=lit, tmax=np.where(lit, dist, F(0)).astype(F), mat=mat, tex=tex,
               light=light, pos=pos, dnl0=dnl0, fell=fell_px, nfall=nfall, attributes=attributes)


def linear(P, sv, sm, pow64=True):
    """the float32 colour before the gamma and the shadow flag.  pow64: the specular powf in float64 from its float32 arguments, rounded to
    float32 (False: numpy's float32 power, which makes this attr_ref.shade / render_ref.shade up to the gamma)"""
    _, intensity, ltype = P.light
    kind, N, L, dist, mat, d = P.kind, P.N, P.L, P.dist, P.mat, P.d
    tri = kind == 2
    with np.errstate(all="ignore"):
        li = np.full(P.n, F(intensity), F) if ltype == 1 else F(intensity) / (dist * dist)
        dnl = np.fmax(P.dnl0, F(0))
        diff = mat["diffuse"] * dnl[:, None]
        diff = np.where((mat["illum"] >= 1)[:, None], diff + mat["ambient"], diff)
        if P.attributes:
            diff = np.where(tri[:, None], diff * P.tex, diff).astype(F)
        lit = P.dnl0 > 0
        sh = lit & ((np.asarray(sv) != 0) | (np.asarray(sm) != 0))
        att = np.where(lit, np.where(sh, F(0.3), F(1)), np.where(tri, F(1), F(0.3))).astype(F)
        spec = np.zeros_like(diff)
        s = lit & ~sh & (mat["illum"] >= 2) & (kind > 0)
        if s.any():
            kSh = np.fmax(mat["shininess"][s], F(4))
            kE = (F(2) + kSh) / (F(2) * F(3.14159265))
            e = d[s] * F(-1)
            V = e / np.sqrt(_dot(e, e))[:, None]
            I = L[s] * F(-1)
            Rr = I - N[s] * (F(2) * _dot(N[s], I))[:, None]
            base = np.fmax(_dot(V, Rr), F(0))
            pw = np.power(base.astype(np.float64), kSh.astype(np.float64)).astype(F) if pow64 else np.power(base, kSh)
            spec[s] = mat["specular"][s] * (kE * pw)[:, None]
        c = ((li * att)[:, None] * (diff + spec)).astype(F)
        c[kind == 0] = render_ref.MISS
    return c, (sh & (kind > 0)).astype(np.uint8)


def expected(P, sv, sm):
    """-> dict(y float64 [n, 3] = 255 * clamp(c)^(1/2.2), byte = floor(y + 0.5), c (float32, before the gamma), kind, shadowed)"""
    c, sh = linear(P, sv, sm)
    with np.errstate(all="ignore"):
        cl = np.fmin(np.fmax(c, F(0)), F(1)).astype(np.float64)                     # fmaxf / fminf: NaN -> 0, +Inf -> 1, negatives -> 0
        y = 255.0 * np.power(cl, GAMMA_EXP)
    return dict(y=y, byte=np.floor(y + 0.5).astype(np.int64), c=c, kind=P.kind, shadowed=sh)


def tie_distance(y):
    return np.abs(y - np.floor(y) - 0.5)


def frame_stats(exp, m=M_TIE):
    """the two conditions that keep the rule from hiding failures, from the expectation alone"""
    hit = exp["kind"] > 0
    near = tie_distance(exp["y"][hit]) < m
    return dict(near_share=float(near.mean()) if hit.any() else 0.0, distinct=int(np.unique(exp["byte"][hit]).size), hits=int(hit.sum()))


def check_stats(exp, flat=None, what=""):
    st = frame_stats(exp)
    assert st["hits"] > 0, what + ": no hit pixel"
    assert st["near_share"] <= NEAR_SHARE_MAX, "%s: %.4f of the channels lie within the margin of a tie" % (what, st["near_share"])
    if flat is None:
        assert st["distinct"] >= DISTINCT_MIN, "%s: only %d distinct byte values" % (what, st["distinct"])
    return st


def compare(out, exp, m=M_TIE, what=""):
    """the device frame `out` (rgba [.., 4], kind, shadowed) against expected(): kind, shadowed, alpha and miss pixels exact; a channel of a
    hit pixel exact where y is at least m from a tie, within 1 elsewhere.  -> dict(max_tie: the largest distance from a tie at which a byte
    differs from floor(y + 0.5) (inf for a difference above 1), differing: how many do)"""
    n = len(exp["kind"])
    rgba = np.asarray(out["rgba"]).reshape(n, 4)
    assert np.array_equal(np.asarray(out["kind"]).ravel(), exp["kind"]), what + ": kind differs"
    assert np.array_equal(np.asarray(out["shadowed"]).ravel(), exp["shadowed"]), what + ": shadowed differs"
    assert (rgba[:, 3] == 255).all(), what + ": alpha"
    miss = exp["kind"] == 0
    assert (rgba[miss] == np.uint8(MISS_RGBA)).all(), what + ": miss colour"
    hit = ~miss
    diff = rgba[hit, :3].astype(np.int64) - exp["byte"][hit]
    td = tie_distance(exp["y"][hit])
    off = diff != 0
    max_tie = float(np.where(np.abs(diff) > 1, np.inf, td)[off].max()) if off.any() else 0.0
    bad = np.where(td >= m, off, np.abs(diff) > 1)
    if bad.any():
        r, ch = np.argwhere(bad)[0]
        px = np.flatnonzero(hit)[r]
        raise AssertionError("%s: %d channels differ away from a tie (margin %.3g), first pixel %d channel %d: device %d, y = %.9f, c = %r"
                             % (what, int(bad.sum()), m, px, ch, rgba[px, ch], exp["y"][px, ch], exp["c"][px, ch]))
    return dict(max_tie=max_tie, differing=int(off.sum()))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
UNLIT = (F([0.0, 0.0, 1.0]), F(1.0), 1)               # a directional light behind the sheet: dot(N, L) = -1 in both modes, L exact
FRONT = (F([0.0, 3.0, -4.0]), F(1.0), 1)              # directional, |position| = 5 exactly: L = (0, 0.6, -0.8) rounded
POINT = (F([2.0, 3.0, -12.0]), F(150.0), 0)


def _case(name, sh, mesh, light, modes=(False, True), flat=None, **kw):
    return _ns(name=name, sh=sh, mesh=mesh, light=light, modes=modes, flat=flat, **kw)


def inverse_gamma(y):
    """the float32 c nearest to the one whose 255 * c^(1/2.2) is y (float64 search over the neighbours of the analytic inverse)"""
    c0 = F((y / 255.0) ** (1.0 / GAMMA_EXP))
    cand = [c0]
    lo = hi = c0
    for _ in range(4):
        lo, hi = np.nextafter(lo, F(-1)), np.nextafter(hi, F(2))
        cand += [lo, hi]
    cand = np.array(cand, F)
    return cand[np.argmin(np.abs(255.0 * cand.astype(np.float64) ** GAMMA_EXP - y))]


GAMMA_SPECIALS = (F(0.0), F(-0.0), SUBNORMAL, F(1.0), np.nextafter(F(1), F(2)), F(1e30), F(np.inf), F(-np.inf), F(np.nan), F(-1.0))


@functools.lru_cache(maxsize=None)
def gamma_values():
    """the float32 values nearest to y = k + 0.5 -/+ 2 m for each of the 255 byte boundaries (off the tie on both sides: exact), then the
    specials"""
    v = []
    for k in range(255):
        v += [inverse_gamma(k + 0.5 - 2 * M_TIE), inverse_gamma(k + 0.5 + 2 * M_TIE)]
    return _frozen(np.array(v + list(GAMMA_SPECIALS), F))


@functools.lru_cache(maxsize=None)
def case_gamma():
    """an unlit triangle with an illum 1 material under a directional light of intensity 1: c = (1*1) * (diffuse*0 + ambient) = ambient"""
    sh = sheet(32, 16)
    v = gamma_values()
    q = np.arange(sh.nq)
    amb = np.stack([v[q % len(v)], v[(q * 7 + 3) % len(v)], v[(q * 11 + 259) % len(v)]], 1)
    mats = np.zeros(sh.nq, MATERIAL)
    mats["ambient"], mats["diffuse"], mats["illum"], mats["shininess"] = amb, F(0.5), 1, F(8)
    mesh = spec_mesh(sh.verts, sh.tris, mats=mats, ids=np.repeat(q, 2).astype(np.int32))
    return _case("gamma", sh, mesh, UNLIT, ambient=_frozen(amb))


@functools.lru_cache(maxsize=None)
def srgb_image():
    """16 x 16: R, G and B each run through all 256 bytes, in three different orders; alpha random"""
    rng = np.random.default_rng(11)
    i = np.arange(256)
    img = np.stack([i, (i * 37 + 11) % 256, 255 - (i * 101) % 256, rng.integers(0, 256, 256)], 1).astype(np.uint8)
    assert all(np.unique(img[:, c]).size == 256 for c in range(3))
    return _frozen(img.reshape(16, 16, 4))


@functools.lru_cache(maxsize=None)
def case_srgb():
    """the unlit geometry with ambient 1: c = the bilinear blend of table entries.  Quad (i, j), i < 16: the centre of texel (i, j) of the
    16 x 16 image; columns 16, 17: 1 x 1 textures of the table's end points and their neighbours"""
    sh = sheet(18, 16)
    q = np.arange(sh.nq)
    i, j = q % 18, q // 18
    uv = np.stack([(np.minimum(i, 15) + 0.5) / 16.0, (j + 0.5) / 16.0], 1)
    ends = [(0, 0, 0), (255, 255, 255), (0, 255, 1), (254, 1, 255), (1, 1, 1), (10, 11, 12), (11, 10, 254), (128, 127, 129)]    # 10 / 11: the EOTF's knee
    images = [srgb_image()] + [np.uint8([[list(e) + [7]]]) for e in ends]
    mats = np.zeros(1 + len(ends), MATERIAL)
    mats["ambient"], mats["diffuse"], mats["illum"] = F(1), F(0.5), 1
    ids = np.where(i < 16, 0, 1 + (j + 16 * (i - 16)) % len(ends))
    mesh = spec_mesh(sh.verts, sh.tris, cuv=per_quad(uv.astype(F)), mats=mats, ids=np.repeat(ids, 2).astype(np.int32),
                     slots=np.arange(1 + len(ends), dtype=np.int32), images=images)
    return _case("srgb", sh, mesh, UNLIT, modes=(True,))


TEX_SIZES = ((1, 1), (1, 7), (7, 1), (2, 2), (37, 19), (16384, 1), (1, 16384))


@functools.lru_cache(maxsize=None)
def tex_images():
    rng = np.random.default_rng(23)
    return tuple(_frozen(rng.integers(0, 256, (h, w, 4)).astype(np.uint8)) for w, h in TEX_SIZES)


def _x_of(u, w):
    with np.errstate(all="ignore"):
        return F(u) * F(w) - F(0.5)


def _u_for(target, w, side):
    """the float32 u whose x = u*w - 0.5 is the nearest to `target` from below (side -1: x <= target) or from above (+1: x >= target)"""
    u = F((target + 0.5) / w)
    cand = [u]
    lo = hi = u
    for _ in range(6):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        cand += [lo, hi]
    cand = np.array(cand, F)
    x = _x_of(cand, w).astype(np.float64)
    ok = x <= target if side < 0 else x >= target
    return cand[ok][np.argmin(np.abs(x[ok] - target))]


def axis_values(w):
    """(name, u at the quad's low edge, u at its high edge) per probe of one axis of a texture of extent w"""
    T31, T62 = 2.0 ** 31, 2.0 ** 62
    below62 = float(np.nextafter(F(T62), F(0)))
    out = [("x in -1..0", (-1 + 0.5) / w, (0 + 0.5) / w), ("x in 0..1", 0.5 / w, 1.5 / w),
           ("x = 3", 3.5 / w, 3.5 / w), ("x = -3", -2.5 / w, -2.5 / w), ("x = 0", 0.5 / w, 0.5 / w),
           ("last of 32 bits +", _u_for(T31 - 128, w, -1), _u_for(T31 - 128, w, -1)), ("first of 64 bits +", _u_for(T31, w, +1), _u_for(T31, w, +1)),
           ("last of 32 bits -", _u_for(-(T31 - 128), w, +1), _u_for(-(T31 - 128), w, +1)), ("first of 64 bits -", _u_for(-T31, w, -1), _u_for(-T31, w, -1)),
           ("2^40 scale +", 1.37 * 2.0 ** 40 / w, 1.38 * 2.0 ** 40 / w), ("2^40 scale -", -1.38 * 2.0 ** 40 / w, -1.37 * 2.0 ** 40 / w),
           ("below 2^62", _u_for(below62, w, -1), _u_for(below62, w, -1)), ("2^62", _u_for(T62, w, +1), _u_for(T62, w, +1)),
           ("below -2^62", _u_for(-below62, w, +1), _u_for(-below62, w, +1)),
           ("FLT_MAX", FLT_MAX, FLT_MAX), ("-FLT_MAX", -FLT_MAX, -FLT_MAX), ("+Inf", np.inf, np.inf), ("-Inf", -np.inf, -np.inf), ("NaN", np.nan, np.nan),
           ("x in -40..40", -39.5 / w, 40.5 / w)]
    return [(nm, F(a), F(b)) for nm, a, b in out]


NPROBE = 20


@functools.lru_cache(maxsize=None)
def case_texture(sloped):
    """quad ((t*2 + axis)*NPROBE + p): texture t, probe p of axis_values on the u (axis 0) or v (axis 1) axis; the other axis is the constant
    0.3 (sloped False) or runs from -0.3 to 1.7 across the quad (True).  Lit by FRONT through an illum 1 material"""
    sh = sheet(24, 12)
    imgs = tex_images()
    assert len(TEX_SIZES) * 2 * NPROBE <= sh.nq
    cuv = np.zeros((sh.nt, 3, 2), F)
    ids = np.full(sh.nq, len(TEX_SIZES), np.int64)                                    # the spare quads: an untextured material
    names = {}
    st = sh.corner.reshape(sh.nq, 2, 3, 2).astype(np.float64)
    for t, (w, h) in enumerate(TEX_SIZES):
        for axis in (0, 1):
            vals = axis_values((w, h)[axis])
            assert len(vals) == NPROBE
            for p, (nm, a, b) in enumerate(vals):
                q = (t * 2 + axis) * NPROBE + p
                names[q] = (t, axis, nm)
                ids[q] = t
                s = st[q, :, :, axis]                                                  # the quad coordinate along the probed axis
                if a == b or not (np.isfinite(a) and np.isfinite(b)):
                    probe = np.full((2, 3), a, F)
                else:
                    probe = (np.float64(a) + (np.float64(b) - np.float64(a)) * s).astype(F)
                other = (-0.3 + 2.0 * st[q, :, :, 1 - axis]).astype(F) if sloped else np.full((2, 3), F(0.3))
                cuv[2 * q:2 * q + 2, :, axis] = probe
                cuv[2 * q:2 * q + 2, :, 1 - axis] = other
    mats = np.zeros(len(TEX_SIZES) + 1, MATERIAL)
    mats["ambient"], mats["diffuse"], mats["illum"] = F([0.05, 0.1, 0.15]), F([0.9, 0.8, 0.7]), 1
    slots = np.int32(list(range(len(TEX_SIZES))) + [-1])
    mesh = spec_mesh(sh.verts, sh.tris, cuv=_frozen(cuv), mats=mats, ids=np.repeat(ids, 2).astype(np.int32), slots=slots, images=list(imgs))
    return _case("texture sloped" if sloped else "texture const", sh, mesh, FRONT, modes=(True,), names=names)


def texture_arms(ma, prim, bary):
    """per triangle pixel and axis the arm of tex_axis its uv takes on its material's texture: 0 the 32-bit residue, 1 the 64-bit residue,
    2 texel 0 / weight 0 (|x| >= 2^62 or non-finite), -1 no texture; and the x itself"""
    prim = np.asarray(prim, np.int64)
    b0, b1, b2 = attr_ref.bary3(bary)
    c = F(ma.cuv).reshape(-1, 3, 2)[prim] if ma.cuv is not None else np.zeros((len(prim), 3, 2), F)
    arms = np.full((len(prim), 2), -1, np.int64)
    xs = np.full((len(prim), 2), np.nan)
    if ma.ids is None or ma.slots is None:
        return arms, xs
    mi = np.asarray(ma.ids, np.int64)[prim]
    ok = (mi >= 0) & (mi < len(ma.slots))
    sl = np.where(ok, np.asarray(ma.slots, np.int64)[np.clip(mi, 0, len(ma.slots) - 1)], -1)
    with np.errstate(all="ignore"):
        uv = attr_ref.interp(c, b0, b1, b2)
        for s, img in enumerate(ma.images):
            k = sl == s
            h, w = (1, 1) if img is None else img.shape[:2]
            for axis, ext in ((0, w), (1, h)):
                x = uv[k, axis] * F(ext) - F(0.5)
                far = ~(np.abs(x) < F(2.0 ** 62))
                wide = ~far & (np.abs(np.floor(x)) >= F(2.0 ** 31))
                arms[k, axis] = np.where(far, 2, np.where(wide, 1, 0))
                xs[k, axis] = x
    return arms, xs


@functools.lru_cache(maxsize=None)
def case_slots():
    """a textured material on a mesh WITHOUT uvs (u = v = 0: x = -0.5, the blend of the four corner texels with weights 1/2), slots -1,
    ntex, INT32_MIN, a slot with no image (magenta), and triangles without a material (id -1)"""
    sh = sheet(8, 4)
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (19, 37, 4)).astype(np.uint8), rng.integers(0, 256, (2, 2, 4)).astype(np.uint8), None,
              rng.integers(0, 256, (1, 7, 4)).astype(np.uint8)]
    slots = np.int32([0, -1, len(images), INT32_MIN, 2, 1, 3, 2 ** 31 - 1])
    mats = np.zeros(len(slots), MATERIAL)
    mats["ambient"], mats["illum"] = F([0.05, 0.1, 0.15]), 1
    mats["diffuse"] = F([[0.9 - 0.05 * k, 0.5 + 0.05 * k, 0.7] for k in range(len(slots))])
    ids = np.arange(sh.nq) % (len(slots) + 1) - 1                                     # -1, 0 .. 7
    mesh = spec_mesh(sh.verts, sh.tris, mats=mats, ids=np.repeat(ids, 2).astype(np.int32), slots=slots, images=images)
    return _case("slots", sh, mesh, FRONT, modes=(True,), flat="u = v = 0 on every pixel: one colour per material")


NORMAL_PROBES = (
    ("tilted", [(0.2, 0.1, -1.0)] * 3, False), ("unit", [(0.0, 0.0, -1.0)] * 3, False), ("zero", [(0.0, 0.0, 0.0)] * 3, True),
    ("nan corner", [(np.nan, 0.1, -1.0), (0.2, 0.1, -1.0), (0.2, 0.1, -1.0)], True), ("+inf corner", [(0.2, 0.1, -1.0), (0.2, np.inf, -1.0), (0.2, 0.1, -1.0)], True),
    ("-inf corner", [(0.2, 0.1, -1.0), (0.2, 0.1, -1.0), (0.2, 0.1, -np.inf)], True), ("1e20", [(0.2e20, 0.1e20, -1e20)] * 3, True),
    ("1e-30", [(0.2e-30, 0.1e-30, -1e-30)] * 3, True), ("1e-20", [(0.2e-20, 0.1e-20, -1e-20)] * 3, False),
    ("n1 = -n0", [(0.2, 0.1, -1.0), (-0.2, -0.1, 1.0), (0.2, 0.1, -1.0)], None), ("back-facing", [(0.1, -0.2, 1.0)] * 3, False),
    ("perpendicular to FRONT", [(1.0, 0.0, 0.0)] * 3, False), ("sloped", [(0.5, 0.0, -1.0), (-0.5, 0.3, -1.0), (0.0, -0.4, -1.0)], False),
    ("1e18 (dot 1e36)", [(0.2e18, 0.1e18, -1e18)] * 3, False), ("FLT_MAX", [(0.0, 0.0, -float(FLT_MAX))] * 3, True),
    ("subnormal", [(0.0, 0.0, -1e-45)] * 3, True))                                    # the third field: does every pixel fall back (None: some)


TINY = (F([3.0, 4.0, -10.0]) * F(1e-30), F(1.0), 1)   # directional, so short that dot(l, l) underflows to 0: len = 0, 1 / len = +Inf, L = (+Inf, +Inf, -Inf)


@functools.lru_cache(maxsize=None)
def case_normals(light):
    """attribute mode: quad q has the corner normals of probe q % 16 and the material q // 16 (illum 1 / illum 2 with a specular term).
    light: False FRONT, True POINT, "tiny" TINY -- the one light under which a LIT pixel has a non-finite shadow ray: where N is non-zero in
    all three components and has L's signs, dot(N, L) = +Inf"""
    sh = sheet(8, 4)
    cn = np.zeros((sh.nt, 3, 3), F)
    for q in range(sh.nq):
        with np.errstate(all="ignore"):
            cn[2 * q:2 * q + 2] = F(NORMAL_PROBES[q % 16][1])[None]
    mats = table([material(0.05, (0.8, 0.6, 0.4), 0.0, 16.0, 1), material((0.02, 0.04, 0.06), (0.5, 0.7, 0.9), 0.6, 6.0, 2)])
    ids = np.arange(sh.nq) // 16
    mesh = spec_mesh(sh.verts, sh.tris, cnrm=_frozen(cn), mats=mats, ids=np.repeat(ids, 2).astype(np.int32))
    name, lt, flat = {False: ("normals directional", FRONT, None), True: ("normals point", POINT, None),
                      "tiny": ("normals tiny directional", TINY, "L is infinite or NaN: a channel is saturated, or ambient only")}[light]
    return _case(name, sh, mesh, lt, modes=(True,), flat=flat)


ILLUMS = (-1, 0, 1, 2, 3, 7)
SHININESS = (0.0, 3.999, 4.0, 1000.0, 1e30, np.inf, np.nan)
COLOURS = (-0.5, 5.0, 1e30)


def material_table(finite_only=False):
    """illum x Ns, then diffuse / ambient / specular with one component of -0.5, 5 and 1e30 each; finite_only: without the Inf and NaN Ns (the
    voxel path de-duplicates materials by operator==)"""
    recs = []
    for il in ILLUMS:
        for ns in SHININESS:
            if finite_only and not np.isfinite(ns):
                continue
            recs.append(material((0.03, 0.05, 0.07), (0.7, 0.5, 0.3), (0.9, 0.8, 0.7), ns, il))
    for f in ("diffuse", "ambient", "specular"):
        for k, cval in enumerate(COLOURS):
            r = material((0.03, 0.05, 0.07), (0.7, 0.5, 0.3), (0.9, 0.8, 0.7), 8.0, 2)
            r[f][0, k] = F(cval)
            recs.append(r)
        r = material((0.03, 0.05, 0.07), (0.7, 0.5, 0.3), (0.9, 0.8, 0.7), 8.0, 2)
        r[f] = F(COLOURS)
        recs.append(r)
    return table(recs)


@functools.lru_cache(maxsize=None)
def case_materials():
    """16 x 8 quads: quad q has material q % (n + 1) - 1 of material_table() (-1: no material, MaterialObj{}); the highlight of POINT (or of
    any light on the camera's side) lies on the sheet"""
    sh = sheet(16, 8)
    mats = material_table()
    ids = np.arange(sh.nq) % (len(mats) + 1) - 1
    mesh = spec_mesh(sh.verts, sh.tris, mats=mats, ids=np.repeat(ids, 2).astype(np.int32))
    return _case("materials", sh, mesh, POINT)


@functools.lru_cache(maxsize=None)
def slab():
    """the voxel source of the material and light cases: two 5 x 6 sheets of unit quads at z = -2.5 and z = -2 over the camera-left part of the
    frame, one finite material per quad (the same on both sheets); voxelized at 0.25 it is a thin slab, well inside 32^3 cells, whose shadow falls
    on the probe sheet"""
    Q, R = 5, 6
    i, j = np.meshgrid(np.arange(Q), np.arange(R))
    st = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)
    verts = np.zeros((2, Q * R, 4, 3))
    verts[:, :, :, 0] = (i.ravel() + 1.5)[None, :, None] + st[None, None, :, 0]
    verts[:, :, :, 1] = (j.ravel() - R / 2.0)[None, :, None] + st[None, None, :, 1]
    verts[0, :, :, 2], verts[1, :, :, 2] = -2.5, -2.0
    base = 4 * np.arange(2 * Q * R)[:, None]
    tris = np.stack([base + [0, 2, 1], base + [0, 3, 2]], 1).reshape(-1, 3)
    mats = material_table(finite_only=True)
    ids = np.repeat(np.tile(np.arange(Q * R) * 5 % len(mats), 2), 2)
    return _ns(verts=_frozen(verts.reshape(-1, 3).astype(F)), tris=_frozen(tris.astype(np.int32)), mats=mats, ids=_frozen(ids.astype(np.int32)),
               voxel_size=F(0.25))


BASE_DIR = (3.0, 4.0, -10.0)
LIGHTS = {
    # point lights
    "point 1e-3 from the sheet": (F([0.3, 0.2, -1e-3]), F(1.0), 0),
    "point at 1e18": (F([0.3e18, 0.2e18, -1e18]), F(1000.0), 0),                      # li = 1000 / 1.13e36: every byte 0
    "point at 1e18, intensity 1e36": (F([0.3e18, 0.2e18, -1e18]), F(1e36), 0),        # ... and the same light made visible
    "point at 1e20": (F([0.3e20, 0.2e20, -1e20]), F(1000.0), 0),                      # dot(l, l) overflows: len = Inf, L = 0, li = 0
    "point in the sheet's plane": (F([20.0, 0.0, 0.0]), F(400.0), 0),                 # dot(N, L) = -0 on the triangles
    "point behind the sheet": (F([1.0, 2.0, 10.0]), F(100.0), 0),
    # intensities
    "intensity 0": (POINT[0], F(0.0), 0), "intensity -1": (POINT[0], F(-1.0), 0), "intensity 1e30": (POINT[0], F(1e30), 0),
    "intensity subnormal": (F(BASE_DIR), SUBNORMAL, 1), "directional intensity -1": (F(BASE_DIR), F(-1.0), 1),
    # directional lights
    "directional": (F(BASE_DIR), F(1.0), 1),
    "directional * 1e-30": (F(BASE_DIR) * F(1e-30), F(1.0), 1),                       # dot underflows to 0: len = 0, inv = Inf, dot(N, L) NaN
    "directional * 1e30": (F(BASE_DIR) * F(1e30), F(1.0), 1),                         # dot overflows: L = 0
    "directional (0, 0, 0)": (F([0.0, 0.0, 0.0]), F(1.0), 1),
    "directional NaN component": (F([np.nan, 4.0, -10.0]), F(1.0), 1),
    "directional +Inf component": (F([3.0, np.inf, -10.0]), F(1.0), 1),
    "point NaN component": (F([2.0, np.nan, -12.0]), F(150.0), 0),
    "point -Inf component": (F([2.0, 3.0, -np.inf]), F(150.0), 0),
    "intensity NaN": (POINT[0], F(np.nan), 0), "intensity +Inf": (F(BASE_DIR), F(np.inf), 1),
}
# the lights whose frame is one flat colour (or black), and why
FLAT_LIGHTS = {
    "point at 1e18": "li = 1000 / 1.13e36", "point at 1e20": "li = 0", "intensity 0": "li = 0", "intensity -1": "every colour negative or -0",
    "intensity subnormal": "li = 2^-149", "directional * 1e-30": "unlit: ambient only",
    "directional * 1e30": "unlit: ambient only", "directional (0, 0, 0)": "unlit: ambient only", "directional NaN component": "unlit: ambient only",
    "directional +Inf component": "unlit: ambient only", "point NaN component": "dist NaN: li NaN", "point -Inf component": "li = 0",
    "intensity NaN": "li NaN", "intensity +Inf": "every lit channel saturates", "intensity 1e30": "every lit channel saturates",
}
# the lights under which dot(N, L) is NaN on every hit pixel of the flat-normal sheets (N = (0, 0, -1) exactly)
NAN_DOT_LIGHTS = ("directional * 1e-30", "directional (0, 0, 0)", "directional NaN component", "directional +Inf component", "point NaN component",
                  "point -Inf component")


def light_on_pixel(P, px):
    """a point light on the bit pattern of pixel px's own hit position (l = 0 there: L is NaN on that pixel only)"""
    assert P.kind[px] == 2
    return (P.pos[px].copy(), F(1.0), 0)


# ---- the instanced scene ----------------------------------------------------------------------------------------------------------------
def _rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _object_space(xf, world):
    """the float32 object coordinates whose image under the 3x4 transform xf is (about) the world vertices"""
    m = np.asarray(xf, np.float64).reshape(3, 4)
    return (np.linalg.inv(m[:, :3]) @ (np.asarray(world, np.float64) - m[:, 3]).T).T.astype(F)


@functools.lru_cache(maxsize=None)
def case_instanced():
    """three 8 x 8 sheets side by side in one 24 x 8 frame, one BLAS and one instance each, in the BLAS order [bare; corner normals,
    materials and textures but no uvs; uvs, textures and materials but no corner normals].  The last one -- the face-normal path -- stands under
    a rotated, mirrored transform scaled by (1e-3, 1, 1e3).  Every BLAS has its own material table, slot table and texture sizes.  Object
    vertices are the inverse images of the world sheets, so the picture is still the head-on sheet."""
    parts = [sheet(8, 8, x0=-8.0, total_q=24), sheet(8, 8, x0=0.0, total_q=24), sheet(8, 8, x0=8.0, total_q=24)]
    xfs = [instance_ref.transform(rot=_rot((1, 2, 3), 20.0), scale=(1.0, 1.0, 1.0), offset=(0.3, -0.2, 0.1)),
           instance_ref.transform(rot=_rot((0, 0, 1), 90.0), scale=(2.0, 0.5, 1.0), offset=(0.0, 0.0, 0.0)),
           instance_ref.transform(rot=_rot((3, -1, 2), 40.0), scale=(-1e-3, 1.0, 1e3), offset=(1.0, 2.0, -3.0))]
    rng = np.random.default_rng(31)
    meshes = []
    # BLAS 0: bare
    meshes.append(spec_mesh(_frozen(_object_space(xfs[0], parts[0].verts)), parts[0].tris))
    # BLAS 1: corner normals (object space: tilted, sloped and falling back), materials, textures without uvs
    sh = parts[1]
    cn = np.zeros((sh.nt, 3, 3), F)
    for q in range(sh.nq):
        with np.errstate(all="ignore"):
            cn[2 * q:2 * q + 2] = F(NORMAL_PROBES[q % 16][1])[None]
    m1 = table([material(0.05, (0.8, 0.6, 0.4), 0.0, 16.0, 1), material((0.02, 0.04, 0.06), (0.5, 0.7, 0.9), 0.6, 6.0, 2),
                material(0.1, 0.9, 0.2, 2.0, 3)])
    meshes.append(spec_mesh(_frozen(_object_space(xfs[1], sh.verts)), sh.tris, cnrm=_frozen(cn), mats=m1,
                            ids=np.repeat(np.arange(sh.nq) % 4 - 1, 2).astype(np.int32), slots=np.int32([1, -1, 0]),
                            images=[rng.integers(0, 256, (1, 7, 4)).astype(np.uint8), rng.integers(0, 256, (7, 1, 4)).astype(np.uint8)]))
    # BLAS 2: uvs, textures and materials, no corner normals: the face normal through W^T of the scaled, mirrored instance
    sh = parts[2]
    st = sh.corner.astype(np.float64)
    q3 = np.repeat(np.arange(sh.nq), 2)[:, None]
    cuv = np.stack([-1.3 + 0.5 * (q3 % 8) + 0.9 * st[:, :, 0], 2.6 - 0.6 * (q3 // 8) - 1.1 * st[:, :, 1]], 2).astype(F)
    m2 = table([material((0.05, 0.1, 0.15), (0.9, 0.8, 0.7), 0.0, 16.0, 1), material(0.05, 0.8, 0.5, 5.0, 2), material(0.1, 0.6, 0.0, 1.0, 0),
                material(0.2, 0.5, 0.9, 40.0, 7)])
    meshes.append(spec_mesh(_frozen(_object_space(xfs[2], sh.verts)), sh.tris, cuv=_frozen(cuv), mats=m2,
                            ids=np.repeat(np.arange(sh.nq) % 5 - 1, 2).astype(np.int32), slots=np.int32([2, 0, 5, 1]),
                            images=[rng.integers(0, 256, (19, 37, 4)).astype(np.uint8), rng.integers(0, 256, (2, 2, 4)).astype(np.uint8),
                                    rng.integers(0, 256, (3, 5, 4)).astype(np.uint8)]))
    inst = instance_ref.make_instances(xfs, blas=[0, 1, 2])
    cam = sheet(24, 8).cam
    return _ns(name="instanced", meshes=meshes, inst=inst, cam=cam, W=cam[2], H=cam[3], light=POINT)


@functools.lru_cache(maxsize=None)
def cpu_trace_instanced():
    c = case_instanced()
    vi, pi, W, H = c.cam
    d = render_ref.host_dirs(vi, pi, W, H)
    rays = np.concatenate([np.tile(F(vi[12:15]), (W * H, 1)), d], 1)
    host = [(m.verts, m.tris) for m in c.meshes]
    t, ii, pp, bb = instance_ref.closest(host, c.inst, rays)
    return dict(t=_frozen(t), instance=_frozen(ii), prim=_frozen(pp), bary=_frozen(bb), normal=_frozen(instance_ref.world_normals(host, c.inst, ii, pp)))


def cpu_frame(case, attributes, light=None, pow64=True):
    """prepare() + expected() over the CPU brute force of a sheet case, without shadows (one planar sheet casts none on itself)"""
    mo = cpu_trace(case.sh.Q, case.sh.R, case.sh.px)
    P = prepare(case.sh.cam, None, mo, [case.mesh], light or case.light, attributes)
    z = np.zeros(P.n, np.uint8)
    return P, expected(P, z, z), mo
