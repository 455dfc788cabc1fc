"""The inputs of tests/shading_extremes.py do what they claim, on the restatements alone (no GPU): every case reaches the arm it names, the
frames meet the two conditions that keep "exact away from ties" from hiding failures, the high-precision evaluation is the restatements'
arithmetic up to the two powf calls, and compare() rejects what it should.  Traversal inputs: tests/mesh_ref.py's brute force on the sheets."""
import numpy as np
import pytest

import attr_ref
import instance_ref
import render_ref
import shading_extremes as sx

F = np.float32
SHEET_CASES = [(sx.case_gamma, None), (sx.case_srgb, None), (sx.case_texture, False), (sx.case_texture, True), (sx.case_slots, None),
               (sx.case_normals, False), (sx.case_normals, True), (sx.case_normals, "tiny"), (sx.case_materials, None)]


def get(fn, arg):
    return fn() if arg is None else fn(arg)


def restated_bytes(case, P, attributes):
    """attr_ref.shade / render_ref.shade on the same inputs"""
    z = np.zeros(P.n, np.uint8)
    mo = sx.cpu_trace(case.sh.Q, case.sh.R, case.sh.px)
    vn = np.zeros((P.n, 3), F)
    mmat = {k: v for k, v in P.mat.items()}
    with np.errstate(all="ignore"):
        if attributes:
            return attr_ref.shade(P.d, P.kind, vn, P.N, P.L, P.dist, z, z, P.light, None, mmat, P.tex)
        return render_ref.shade(P.d, P.kind, vn, mo["normal"], P.L, P.dist, z, z, P.light, None, mmat)


def test_material_record_is_the_librarys():
    import voxhip
    assert sx.MATERIAL == voxhip.MATERIAL


@pytest.mark.parametrize("fn,arg", SHEET_CASES)
def test_frames_meet_the_conditions_and_match_the_restatements(fn, arg):
    case = get(fn, arg)
    for attributes in case.modes:
        P, exp, mo = sx.cpu_frame(case, attributes)
        sx.check_stats(exp, case.flat, case.name)
        # the float32 path of linear() is the restatement: the same bytes through numpy's float32 gamma
        c32, sh = sx.linear(P, np.zeros(P.n, np.uint8), np.zeros(P.n, np.uint8), pow64=False)
        rgba, rsh = restated_bytes(case, P, attributes)
        with np.errstate(all="ignore"):
            g = np.power(np.fmin(np.fmax(c32, F(0)), F(1)), F(1.0) / F(2.2))
        assert np.array_equal(np.floor(g * F(255) + F(0.5)).astype(np.uint8), rgba[:, :3]) and np.array_equal(sh, rsh)
        # ... and the restatement passes the comparison it is meant to be held to
        res = sx.compare(dict(rgba=rgba, kind=P.kind, shadowed=rsh), exp, what=case.name)
        assert res["max_tie"] < sx.M_TIE / 8                                          # numpy's float32 powf: far inside the margin


def test_margin_is_within_its_bounds():
    assert 2.0 ** -12 <= sx.M_TIE <= sx.M_TIE_MAX


def test_restatements_encode_non_finite_channels_by_the_rule():
    n = 6
    kind = np.full(n, 2, np.uint8)
    d = np.tile(F([0, 0, 1]), (n, 1))
    N = np.tile(F([0, 0, -1]), (n, 1))
    L = np.tile(F([0, 0, 1]), (n, 1))                                                # unlit: c = ambient
    mm = render_ref.per_pixel_materials(None, None, n)
    mm["illum"][:] = 1
    mm["ambient"][:, 0] = F([np.nan, np.inf, -np.inf, -1.0, 0.5, 2.0])
    z = np.zeros(n, np.uint8)
    light = (F([0, 0, 1]), F(1), 1)
    with np.errstate(all="ignore"):
        a, _ = attr_ref.shade(d, kind, N, N, L, np.ones(n, F), z, z, light, None, mm, None)
        b, _ = render_ref.shade(d, kind, N, N, L, np.ones(n, F), z, z, light, None, mm)
    for rgba in (a, b):
        assert rgba[:, 0].tolist() == [0, 255, 0, 0, int(np.floor(255 * 0.5 ** (1 / 2.2) + 0.5)), 255]
    # a NaN shininess is 4, a NaN dot(N, L) is not lit (attenuation 1 for a triangle, 0.3 for a voxel)
    L2 = np.tile(F([0, 0, -1]), (n, 1))
    for shade, nrm in ((attr_ref.shade, N), (render_ref.shade, N)):
        out = []
        for ns in (F(np.nan), F(4)):
            m2 = render_ref.per_pixel_materials(None, None, n)
            m2["illum"][:], m2["shininess"][:] = 2, ns
            with np.errstate(all="ignore"):
                out.append(shade(d, kind, nrm, nrm, L2, np.ones(n, F), z, z, (F([0, 0, -1]), F(0.2), 1), None, m2)[0])
        assert np.array_equal(out[0], out[1]) and out[0][:, 2].max() > 0
        Ln = np.tile(F([np.nan, 0, -1]), (n, 1))
        k2 = np.uint8([2, 2, 2, 1, 1, 1])
        m3 = render_ref.per_pixel_materials(None, None, n)
        m3["illum"][:] = 1
        with np.errstate(all="ignore"):
            rgba, sh = shade(d, k2, nrm, nrm, Ln, np.ones(n, F), np.ones(n, np.uint8), np.ones(n, np.uint8), (F([0, 0, -1]), F(1), 1), m3, m3)
        assert not sh.any()
        want = [int(np.floor(255 * float(F(a) * F(0.1)) ** (1 / 2.2) + 0.5)) for a in (1.0, 0.3)]       # diffuse*0 + ambient 0.1, times att
        assert rgba[:3, 0].tolist() == [want[0]] * 3 and rgba[3:, 0].tolist() == [want[1]] * 3


# ---- the cases reach the arms they name ------------------------------------------------------------------------------------------------
def test_gamma_sheet_brackets_every_byte_boundary():
    case = sx.case_gamma()
    v = sx.gamma_values()
    y = 255.0 * np.power(np.clip(v[:510].astype(np.float64), 0, 1), sx.GAMMA_EXP)
    k = np.repeat(np.arange(255), 2)
    off = y - (k + 0.5)
    assert (off[0::2] < 0).all() and (off[1::2] > 0).all()                           # one value on each side of each of the 255 ties
    assert (np.abs(np.abs(off) - 2 * sx.M_TIE) < 0.25 * sx.M_TIE).all()             # float32 spacing is far below the margin
    assert np.array_equal(np.floor(y + 0.5)[0::2], np.arange(255)) and np.array_equal(np.floor(y + 0.5)[1::2], np.arange(1, 256))
    for attributes in (False, True):
        P, exp, mo = sx.cpu_frame(case, attributes)
        tri = P.kind == 2
        assert tri.sum() > 32000 and not P.lit.any() and (P.dnl0[tri] == -1).all()
        amb = case.ambient[sx.quad_of(mo["prim"][tri])]
        assert np.array_equal(exp["c"][tri], amb, equal_nan=True)
        assert sx.tie_distance(exp["y"][tri]).min() >= 1.5 * sx.M_TIE
        seen = np.unique(amb[~np.isnan(amb)])
        assert np.isin(v[~np.isnan(v)], seen).all() and np.isnan(amb).any()          # every value is on the picture
        assert np.isnan(exp["c"][tri]).sum() > 100 and (exp["c"][tri] == np.inf).sum() > 50 and (exp["c"][tri] < 0).sum() > 200


def test_srgb_sheet_samples_every_table_entry_at_its_texel_centre():
    case = sx.case_srgb()
    P, exp, mo = sx.cpu_frame(case, True)
    tri = np.flatnonzero(P.kind == 2)
    q = sx.quad_of(mo["prim"][tri])
    main = q % 18 < 16
    arms, xs = sx.texture_arms(case.mesh, mo["prim"][tri], mo["bary"][tri])
    assert (arms[main] == 0).all() and np.abs(xs[main] - np.round(xs[main])).max() < 1e-4
    img = sx.srgb_image()
    tex = np.round(xs[main]).astype(int) % 16
    for c in range(3):
        assert np.unique(img[tex[:, 1], tex[:, 0], c]).size == 256
        assert np.abs(P.tex[tri][main][:, c] - attr_ref.SRGB[img[tex[:, 1], tex[:, 0], c]]).max() < 4e-6
    assert not P.lit.any() and np.array_equal(exp["c"][tri], P.tex[tri])


@pytest.mark.parametrize("sloped", [False, True])
def test_texture_sheet_reaches_every_arm(sloped):
    case = sx.case_texture(sloped)
    P, exp, mo = sx.cpu_frame(case, True)
    tri = np.flatnonzero(P.kind == 2)
    q = sx.quad_of(mo["prim"][tri])
    arms, xs = sx.texture_arms(case.mesh, mo["prim"][tri], mo["bary"][tri])
    counts = {a: int((arms == a).sum()) for a in (0, 1, 2)}
    print("pixels x axes per arm (32-bit, 64-bit, beyond 2^62 or non-finite):", counts)
    assert counts[1] > 3000 and counts[2] > 3000 and counts[0] > 10000
    want = {"x in -1..0": 0, "x in 0..1": 0, "x = 3": 0, "x = -3": 0, "x = 0": 0, "last of 32 bits +": 0, "last of 32 bits -": 0, "first of 64 bits +": 1,
            "first of 64 bits -": 1, "2^40 scale +": 1, "2^40 scale -": 1, "below 2^62": 1, "below -2^62": 1, "2^62": 2, "FLT_MAX": 2, "-FLT_MAX": 2,
            "+Inf": 2, "-Inf": 2, "NaN": 2, "x in -40..40": 0}
    for quad, (t, axis, name) in case.names.items():
        k = q == quad
        assert k.sum() >= 16, (quad, name)
        x = xs[k, axis]
        w = sx.TEX_SIZES[t][axis]
        # the interpolation (u*b0 + u*b1) + u*b2 of a constant u moves it by an ulp from pixel to pixel: a probe ON a threshold has pixels
        # on both sides of it, and must have some on the side it names
        edge = {"last of 32 bits +": (0, 1), "last of 32 bits -": (0, 1), "first of 64 bits +": (1, 0), "first of 64 bits -": (1, 0), "below 2^62": (1, 2),
                "below -2^62": (1, 2), "2^62": (2, 1)}.get(name, (want[name],))
        assert np.isin(arms[k, axis], edge).all() and (arms[k, axis] == want[name]).sum() >= 8, (sx.TEX_SIZES[t], axis, name, np.unique(arms[k, axis]))
        if name == "x in -1..0":
            assert (np.floor(x) == -1).all()
        elif name == "x in 0..1":
            assert (np.floor(x) == 0).all()
        elif name in ("x = 3", "x = -3", "x = 0"):
            assert np.abs(x - {"x = 3": 3, "x = -3": -3, "x = 0": 0}[name]).max() < 1e-5
        elif name.startswith("last of 32 bits"):
            assert (np.abs(np.floor(x)) >= 2.0 ** 31 - 2.0 ** 23).all()
            if w in (1, 2, 16384):
                assert (np.abs(np.floor(x)) == 2.0 ** 31 - 128).any()               # THE last float32 of the arm, where u*w is exact
        elif name.startswith("first of 64 bits"):
            assert (np.abs(np.floor(x)) < 2.0 ** 31 + 2.0 ** 23).all()
            if w in (1, 2, 16384):
                assert (np.abs(np.floor(x)) == 2.0 ** 31).any()
        elif name.startswith("2^40") and w in (7, 37, 19):
            assert np.unique(np.mod(np.floor(x).astype(np.int64), w)).size >= 3           # the residues differ from pixel to pixel
        elif name == "below 2^62" and w in (1, 2, 16384):
            assert (x == float(np.nextafter(F(2.0 ** 62), F(0)))).any()
        elif name == "2^62" and w in (1, 2, 16384):
            assert (x == 2.0 ** 62).any()


def test_slot_sheet():
    case = sx.case_slots()
    P, exp, mo = sx.cpu_frame(case, True)
    tri = np.flatnonzero(P.kind == 2)
    mid = np.asarray(case.mesh.ids)[mo["prim"][tri].astype(np.int64)]
    textured = np.isin(mid, [0, 4, 5, 6])                                            # slots 0, 2 (no image: magenta), 1, 3
    assert (P.tex[tri][~textured] == 1).all() and (mid == -1).sum() > 100
    arms, xs = sx.texture_arms(case.mesh, mo["prim"][tri], mo["bary"][tri])
    assert (xs[textured] == -0.5).all()                                              # u = v = 0: the corner blend, weights 1/2
    mag = P.tex[tri][mid == 4]
    assert (mag[:, 0] == 1).all() and (mag[:, 1] == 0).all() and (mag[:, 2] == 1).all()
    assert np.unique(P.tex[tri][mid == 0], axis=0).shape[0] == 1 and (P.tex[tri][mid == 0] < 1).all()


def test_normal_sheet():
    for point in (False, True):
        case = sx.case_normals(point)
        P, exp, mo = sx.cpu_frame(case, True)
        tri = np.flatnonzero(P.kind == 2)
        probe = sx.quad_of(mo["prim"][tri]) % 16
        fell = P.fell[tri]
        print("normals that fall back:", int(fell.sum()), "of", len(tri))
        for p, (name, _, falls) in enumerate(sx.NORMAL_PROBES):
            k = probe == p
            assert k.sum() >= 100, name
            if falls is not None:
                assert fell[k].all() == falls and fell[k].any() == falls, name
        assert fell.sum() == sum(int((probe == p).sum()) for p, x in enumerate(sx.NORMAL_PROBES) if x[2]) + fell[probe == 9].sum()
        names = [x[0] for x in sx.NORMAL_PROBES]
        flip = tri[probe == names.index("n1 = -n0")]
        assert (P.N[flip, 2] > 0).sum() > 10 and (P.N[flip, 2] < 0).sum() > 10        # n passes through zero inside the triangle
        back = tri[probe == names.index("back-facing")]
        assert not P.lit[back].any() and (P.N[back, 2] > 0).all()
        sub = tri[probe == names.index("1e-20")]
        d = render_ref._dot(F([0.2e-20, 0.1e-20, -1e-20]), F([0.2e-20, 0.1e-20, -1e-20]))
        assert 0 < d < np.finfo(F).tiny and P.lit[sub].all()                         # a subnormal dot(n, n) still normalises
        if point is False:
            perp = tri[probe == names.index("perpendicular to FRONT")]
            assert (P.dnl0[perp] == 0).all() and not P.lit[perp].any() and (P.tmax[perp] == 0).all()


def test_the_one_lit_pixel_with_a_non_finite_shadow_ray():
    case = sx.case_normals("tiny")
    P, exp, mo = sx.cpu_frame(case, True)
    tri = np.flatnonzero(P.kind == 2)
    probe = sx.quad_of(mo["prim"][tri]) % 16
    assert np.array_equal(P.L[tri[0]], F([np.inf, np.inf, -np.inf])) and (P.dist == 100000).all()
    names = [x[0] for x in sx.NORMAL_PROBES]
    tilted = tri[probe == names.index("tilted")]
    assert P.lit[tilted].all() and (P.dnl0[tilted] == np.inf).all() and (exp["byte"][tilted] == 255).all()
    flat = tri[probe == names.index("unit")]                                         # N = (0, 0, -1): 0 * Inf, not lit
    assert np.isnan(P.dnl0[flat]).all() and not P.lit[flat].any()
    assert not np.isfinite(P.rays[P.lit]).all(1).any()
    # the flat-normal sheets never get there: under the same light every pixel is "not lit"
    P2, _, _ = sx.cpu_frame(sx.case_materials(), True, sx.TINY)
    assert not P2.lit.any()


def test_material_sheet():
    case = sx.case_materials()
    mats = case.mesh.mats
    assert set(mats["illum"].tolist()) == set(sx.ILLUMS) and np.isnan(mats["shininess"]).sum() == len(sx.ILLUMS)
    assert (mats["shininess"] < 4).sum() >= 2 * len(sx.ILLUMS) and np.isinf(mats["shininess"]).sum() == len(sx.ILLUMS)
    for attributes in (False, True):
        P, exp, mo = sx.cpu_frame(case, attributes)
        tri = np.flatnonzero(P.kind == 2)
        mid = np.asarray(case.mesh.ids)[mo["prim"][tri].astype(np.int64)]
        assert set(np.unique(mid).tolist()) == set(range(-1, len(mats)))               # every material, and "none", is on the picture
        c = exp["c"][tri]
        with np.errstate(invalid="ignore"):
            counts = dict(nan=int(np.isnan(c).sum()), saturated=int((c > 1).sum()), negative=int((c < 0).sum()))
        print("material sheet channels:", counts)
        assert counts["nan"] > 500 and counts["saturated"] > 500 and counts["negative"] > 50
        assert (P.mat["illum"][tri][mid == -1] == 0).all() and (P.mat["shininess"][tri][mid == -1] == 0).all()


def test_lights_do_what_they_name():
    case = sx.case_materials()
    kinds = []
    for name, light in sx.LIGHTS.items():
        P, exp, mo = sx.cpu_frame(case, False, light)
        sx.check_stats(exp, sx.FLAT_LIGHTS.get(name), name)
        kinds.append(P.kind)
        hit = P.kind > 0
        lit = P.lit & hit
        assert np.isfinite(P.rays[lit]).all() and np.isfinite(P.tmax[lit]).all(), name    # a lit pixel has a finite shadow ray
        assert (P.tmax[~lit] == 0).all()
        if name in sx.NAN_DOT_LIGHTS:
            assert np.isnan(P.dnl0[hit]).all() and not lit.any(), name
        else:
            assert not np.isnan(P.dnl0[hit]).any(), name
        if name in ("point at 1e20", "directional * 1e30"):
            assert (P.L[hit] == 0).all() and not lit.any()
            if name == "point at 1e20":
                assert np.isinf(P.dist[hit]).all() and (exp["byte"][hit] == 0).all()
        if name == "point at 1e18":
            assert np.isfinite(P.dist[hit]).all() and lit[hit].all() and not (exp["c"][hit] > 1e-2).any()
        if name == "point 1e-3 from the sheet":
            assert (exp["byte"][hit] == 255).any(1).sum() > 50
        if name in ("point in the sheet's plane",):
            assert (P.dnl0[hit] == 0).all() and not lit.any()
        if name == "point behind the sheet":
            assert (P.dnl0[hit] < 0).all()
    assert all(np.array_equal(k, kinds[0]) for k in kinds)                           # kind never depends on the light
    P0, _, _ = sx.cpu_frame(case, False, sx.POINT)
    px = int(np.flatnonzero(P0.kind == 2)[4000])
    P, exp, mo = sx.cpu_frame(case, False, sx.light_on_pixel(P0, px))
    assert np.isnan(P.dnl0[px]) and np.isnan(P.dnl0).sum() == 1 and not P.lit[px] and (P.L[px] != P.L[px]).all()
    sx.check_stats(exp, None, "light on a pixel")


def test_instanced_case():
    c = sx.case_instanced()
    mo = sx.cpu_trace_instanced()
    w2o, det = instance_ref.inverse(c.inst["transform"])
    assert det[2] < 0 and np.allclose(sorted(np.linalg.svd(c.inst["transform"][2].reshape(3, 4)[:, :3].astype(np.float64))[1]), [1e-3, 1, 1e3], rtol=1e-5)
    hit = mo["instance"] != instance_ref.MISS
    for b in range(3):
        assert (c.inst["blas"][mo["instance"][hit].astype(np.int64)] == b).sum() > 3000
    sizes = [[None if i is None else i.shape[:2] for i in m.images] for m in c.meshes]
    assert sizes[0] == [] and sizes[1] != sizes[2] and c.meshes[0].mats is None and c.meshes[2].cnrm is None and c.meshes[1].cuv is None
    z = np.zeros(c.W * c.H, np.uint8)
    for attributes in (False, True):
        for light in (sx.POINT, sx.FRONT):
            P = sx.prepare(c.cam, None, mo, c.meshes, light, attributes, None, c.inst, w2o)
            exp = sx.expected(P, z, z)
            sx.check_stats(exp, None, "instanced")
            if attributes:
                with np.errstate(all="ignore"):
                    ref = attr_ref.frame(c.cam, None, mo, c.meshes, z, z, P.rays, P.dist, light, c.inst, w2o)
                sx.compare(ref, exp, what="attr_ref.frame on the instanced case")
                assert P.nfall > 1000


# ---- the comparison bites ---------------------------------------------------------------------------------------------------------------
def test_compare_rejects_one_byte_away_from_a_tie_and_a_wrong_flag():
    case = sx.case_materials()
    P, exp, mo = sx.cpu_frame(case, True)
    good = dict(rgba=np.concatenate([exp["byte"].astype(np.uint8), np.full((P.n, 1), 255, np.uint8)], 1), kind=P.kind.copy(), shadowed=exp["shadowed"].copy())
    assert sx.compare(good, exp)["differing"] == 0
    hit = np.flatnonzero(P.kind > 0)
    far = hit[(sx.tie_distance(exp["y"][hit, 1]) > 0.25) & (exp["byte"][hit, 1] < 255)][0]
    bad = {k: v.copy() for k, v in good.items()}
    bad["rgba"][far, 1] += 1
    with pytest.raises(AssertionError, match="away from a tie"):
        sx.compare(bad, exp)
    for key in ("kind", "shadowed"):
        bad = {k: v.copy() for k, v in good.items()}
        bad[key][far] ^= 1
        with pytest.raises(AssertionError, match=key):
            sx.compare(bad, exp)
    # inside the margin one step is allowed, two are not
    e2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in exp.items()}
    e2["y"][far, 1] = np.floor(e2["y"][far, 1]) + 0.5 + sx.M_TIE / 2
    e2["byte"][far, 1] = np.floor(e2["y"][far, 1] + 0.5)
    ok = {k: v.copy() for k, v in good.items()}
    ok["rgba"][far, 1] = e2["byte"][far, 1] - 1
    assert sx.compare(ok, e2)["max_tie"] == pytest.approx(sx.M_TIE / 2)
    ok["rgba"][far, 1] = e2["byte"][far, 1] - 2
    with pytest.raises(AssertionError):
        sx.compare(ok, e2)


def test_compare_rejects_restated_kernel_mistakes():
    """numpy restatements of mistakes that pass "within 1 LSB": weights quantised to 8 bits, a gamma exponent of 0.4545"""
    case = sx.case_texture(True)
    P, exp, mo = sx.cpu_frame(case, True)
    z = np.zeros(P.n, np.uint8)
    frame = lambda c: dict(rgba=np.concatenate([np.floor(255.0 * np.power(np.clip(np.nan_to_num(c.astype(np.float64), nan=0.0), 0, 1), e) + 0.5).astype(np.uint8),
                                                np.full((P.n, 1), 255, np.uint8)], 1), kind=P.kind, shadowed=z)
    e = sx.GAMMA_EXP
    c, _ = sx.linear(P, z, z)
    sx.compare(frame(c), exp)
    e = float(F(0.4545))
    with pytest.raises(AssertionError, match="away from a tie"):
        sx.compare(frame(c), exp)
    assert np.abs(frame(c)["rgba"][:, :3].astype(int) - exp["byte"]).max() <= 1     # ... which "within 1 LSB" lets through
    e = sx.GAMMA_EXP
    real = attr_ref.tex_axis
    try:
        def quantised(u, w):
            i0, i1, f = real(u, w)
            return i0, i1, (np.floor(f * F(256)) / F(256)).astype(F)
        attr_ref.tex_axis = quantised
        Pq = sx.prepare(case.sh.cam, None, mo, [case.mesh], case.light, True)
    finally:
        attr_ref.tex_axis = real
    cq, _ = sx.linear(Pq, z, z)
    with pytest.raises(AssertionError, match="away from a tie"):
        sx.compare(frame(cq), exp)
