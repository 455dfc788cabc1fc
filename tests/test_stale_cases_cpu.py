"""The cases of the stale-memory tests (tests/stale_cases.py) are what those tests say they are: checked here without a GPU."""
import numpy as np

import components_ref as cr
import distance_ref as dr
import mesh_multihit_cases as mc
import morph_ref as mr
import nearest_ref as nr
import nets_ref
import oracle
import solid_ref
import stale_cases as sc
import surface_ref as sr


def test_box_soup_grids_have_the_stated_dimensions(built):
    for dims in (sc.LARGE, sc.SMALL):
        for seed in (1, 2):
            v, t = sc.soup(dims, seed)
            assert len(t) == sc.SOUP_TRIS[dims]
            words, calls, gi = oracle.build_bool(v, t, sc.SOUP_VS)
            assert tuple(gi["dim"]) == dims and len(words) == sc.nwords(dims)
            assert 0 < int(np.unpackbits(words.view(np.uint8)).sum()) <= calls
    # the large soup is dense, the small one sparse
    big = oracle.build_bool(*sc.soup(sc.LARGE), sc.SOUP_VS)[0]
    small = oracle.build_bool(*sc.soup(sc.SMALL), sc.SOUP_VS)[0]
    assert np.unpackbits(big.view(np.uint8)).sum() > 0.5 * np.prod(sc.LARGE)
    assert np.unpackbits(small.view(np.uint8)).sum() < 0.25 * np.prod(sc.SMALL)


def test_mask_occupancies():
    assert 0.40 <= sc.mask("large_half").mean() <= 0.60
    assert 0.05 <= sc.mask("small_tenth").mean() <= 0.20
    assert not sc.mask("large_empty").any() and sc.mask("large_full").all()
    assert not sc.mask("small_empty").any() and sc.mask("small_full").all()
    for name, cells in sc.mask_cases():
        dims = sc.LARGE if name.startswith("large") else sc.SMALL
        assert cells.shape == dims[::-1] and len(sc.words_of(cells)) == sc.nwords(dims)


def test_large_and_small_differ_where_it_matters():
    assert sc.nwords(sc.LARGE) == 1228 and sc.nwords(sc.SMALL) == 10
    assert sc.live_bits_of_last_word(sc.LARGE) == 6 and sc.live_bits_of_last_word(sc.SMALL) == 27
    assert sc.LARGE[0] % 32 != 0 and sc.SMALL[0] % 32 != 0            # rows start at varying bit offsets
    assert np.prod(sc.LARGE) > 2 * 16384                              # more than two scan tiles of cells
    w = sc.words_of(sc.mask("large_full"))
    assert w[-1] == (1 << 6) - 1 and (w[:-1] == 0xFFFFFFFF).all()
    assert sc.words_of(sc.mask("small_full"))[-1] == (1 << 27) - 1


def test_every_reference_runs_on_every_mask(built):
    for name, cells in sc.mask_cases():
        dims = cells.shape[::-1]
        words = sc.words_of(cells)
        assert np.array_equal(solid_ref.unpack(words, dims), cells)
        sw, hw, nh = solid_ref.fill(words, dims)
        assert nh == int(np.unpackbits(sw.view(np.uint8)).sum()) - int(cells.sum())
        d_out, d_in = dr.edt_sq(cells), dr.edt_sq(~cells)
        assert np.array_equal(d_out, dr.edt_sq_c(cells)) and np.array_equal(d_in, dr.edt_sq_c(~cells))
        assert (d_out == 0).sum() == cells.sum() or not cells.any()
        s = dr.sdf_from(cells, d_out, d_in, sc.VS)
        assert s.shape == cells.shape and s.dtype == np.float32
        for target in (cells, ~cells):
            n = nr.nearest(target)
            assert np.array_equal(n, nr.nearest_c(target))
            assert np.array_equal(nr.dist_sq_of(n), dr.edt_sq(target))
        for op in (mr.DILATE, mr.ERODE, mr.OPEN, mr.CLOSE):
            assert np.array_equal(mr.apply(op, cells, 5), mr.apply_fast(op, cells, 5, c=True)), (name, op)
        assert np.array_equal(mr.seal(cells, 2), mr.seal_fast(cells, 2, c=True))
        verts, tris = sr.surface(cells, np.float32(sc.ORG), sc.VS)[:2]
        sv = nets_ref.surface_smooth(cells, np.float32(sc.ORG), sc.VS, 2, 0.5, -0.53, with_normals=True)
        assert len(sv[0]) == len(verts) and len(sv[1]) == len(tris)
        for c in (6, 26):
            lab, k = cr.label(cells, c)
            assert (lab > 0).sum() == cells.sum() and len(cr.stats(lab, k)) == k
    # the shapes of the mode-switch tests
    sp = sc.sparse_cells(sc.LARGE, 5)
    assert 0 < sp.sum() <= 9
    R = 9                                                              # above the bit path's radius (asserted on the GPU against the library's)
    assert mr.apply_fast(mr.DILATE, sp, R * R, c=True).sum() > sp.sum()


def test_cavity_cells_have_an_interior_that_opens():
    closed, opened = sc.cavity_cells(), sc.cavity_cells(opened=True)
    assert (closed != opened).sum() == 1
    nh_closed = solid_ref.fill(sc.words_of(closed), sc.LARGE)[2]
    nh_opened = solid_ref.fill(sc.words_of(opened), sc.LARGE)[2]
    first = 36 * 17 * 10                                               # the inside of the first box
    assert nh_closed - nh_opened == first and nh_opened > 1000


def test_sliver_mesh_has_ill_conditioned_triangles():
    """the header's rule: the sine of the angle at v0 at most 2^-10, both edges non-zero"""
    c = sc.sliver_case()
    assert mc.ILL_SIN == 2.0 ** -10
    ill = mc.side_listed(c.v, c.t)
    assert 50 < int(ill.sum()) < len(c.t)
    # and rays that accept some of them
    assert len(np.unique(c.hits.ray[ill[c.hits.prim]])) >= 10
