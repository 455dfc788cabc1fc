"""CPU tests of the morphology's contract: the two numpy restatements (tests/morph_ref.py) agree with each other and with scipy.ndimage,
the algebraic properties hold, the holed-box facts hold on the oracle's masks, and the C ABI declares, exports and argument-checks the
entry points without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import morph_ref as mr
import oracle
import solid_ref
import vx_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID_ARG = 1

SHAPES = [(7, 9, 37), (5, 33, 64), (1, 1, 70), (12, 3, 31)]   # [Z, Y, X]
R2S = [0, 1, 2, 3, 4, 5, 8, 9, 14, 27, 50, 100]
DENSITIES = [0.02, 0.3, 0.9]


def masks(shape):
    for k, d in enumerate(DENSITIES):
        yield np.random.default_rng(sum(shape) * 31 + k).random(shape) < d


def ball_array(r2):
    R = mr.radius(r2)
    a = np.arange(-R, R + 1)
    return (a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2) <= r2


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("r2", R2S)
def test_two_forms_agree(shape, r2):
    for m in masks(shape):
        for op in (mr.DILATE, mr.ERODE, mr.OPEN, mr.CLOSE):
            assert np.array_equal(mr.apply(op, m, r2), mr.apply_fast(op, m, r2)), (op, r2)
        assert np.array_equal(mr.seal(m, r2), mr.seal_fast(m, r2))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("r2", R2S)
def test_against_scipy(shape, r2):
    ndi = pytest.importorskip("scipy.ndimage")
    B = ball_array(r2)
    R = mr.radius(r2)
    for m in masks(shape):
        assert np.array_equal(mr.dilate(m, r2), ndi.binary_dilation(m, B))
        assert np.array_equal(mr.dilate(m, r2), np.rint(ndi.distance_transform_edt(~m) ** 2) <= r2 if m.any() else np.zeros_like(m))
        assert np.array_equal(mr.erode(m, r2), ndi.binary_erosion(m, B, border_value=0))
        p = np.pad(m, R)
        assert np.array_equal(mr.close(m, r2), mr.crop(ndi.binary_erosion(ndi.binary_dilation(p, B), B), R))
        assert np.array_equal(mr.open_(m, r2), ndi.binary_opening(m, B))
    m = next(masks(shape))
    assert np.array_equal(mr.seal(m, 0), ndi.binary_fill_holes(m))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("r2", [0, 1, 3, 5, 9, 27])
def test_properties(shape, r2):
    for m in masks(shape):
        c = mr.close(m, r2)
        assert (c | m).sum() == c.sum(), "close is extensive"
        assert np.array_equal(mr.close(c, r2), c), "close is idempotent"
        o = mr.open_(m, r2)
        assert (o & ~m).sum() == 0, "open is a subset"
        assert np.array_equal(mr.open_(o, r2), o), "open is idempotent"
        assert (mr.erode(m, r2) & ~m).sum() == 0 and (m & ~mr.dilate(m, r2)).sum() == 0
    m = next(masks(shape))
    assert np.array_equal(mr.seal(m, 0), m | solid_ref.interior_cells(m))


def test_ball_sizes():
    assert [len(mr.ball(r2)) for r2 in (0, 1, 2, 3, 4)] == [1, 7, 19, 27, 33]
    one = np.zeros((9, 9, 9), bool)
    one[4, 4, 4] = True
    assert np.array_equal(mr.dilate(one, 6)[2:7, 2:7, 2:7], ball_array(6)) and mr.dilate(one, 6).sum() == len(mr.ball(6))
    assert mr.erode(mr.dilate(one, 6), 6).sum() == 1 and mr.erode(np.ones((5, 5, 5), bool), 3).sum() == 27


@pytest.fixture(scope="module")
def holed(built):
    out = {}
    for hole in (0.05, 0.6):
        v, t = vx_scenes.holed_box(hole)
        w, _, gi = oracle.build_bool(v, t, F(0.1))
        out[hole] = solid_ref.unpack(w, gi["dim"])
    return out


def test_holed_box_facts(holed):
    narrow, wide = holed[0.05], holed[0.6]
    assert narrow.shape == wide.shape
    solid = narrow | solid_ref.interior_cells(narrow)
    assert solid.sum() > narrow.sum() and solid_ref.interior_cells(wide).sum() == 0
    for r2 in (0, 1, 5, 9):
        assert np.array_equal(mr.seal_fast(narrow, r2), solid), r2
    s4, s5 = mr.seal_fast(wide, 4), mr.seal_fast(wide, 5)
    assert (s4 & ~wide).sum() < 1000, "r2 = 4 does not seal the 0.6 hole"
    assert (s5 ^ solid).sum() < 100, "r2 = 5 seals it"
    assert np.array_equal(s5, mr.seal(wide, 5))
    # a plain close does not: the hole's cells survive, the inside stays empty
    assert (mr.close_fast(wide, 5) ^ solid).sum() > 1000


# ---- the C ABI, without a GPU ------------------------------------------------------------------------------------------------------
NAMES = ["vx_grid_morph_device", "vx_grid_morph_mask", "vx_grid_morph", "vx_grid_seal", "vx_morph_bit_radius"]


def test_header_declares_and_library_exports(vx):
    src = open(os.path.join(ROOT, "include", "voxhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = ctypes.CDLL(vx.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n + " is not declared"
        assert hasattr(L, n), n + " is not exported"
    for k, n in enumerate(("VX_MORPH_DILATE", "VX_MORPH_ERODE", "VX_MORPH_OPEN", "VX_MORPH_CLOSE")):
        assert re.search(r"#define\s+%s\s+%du\b" % (n, k), src), n
    assert (vx.MORPH_DILATE, vx.MORPH_ERODE, vx.MORPH_OPEN, vx.MORPH_CLOSE) == (0, 1, 2, 3)
    assert 1 <= vx.morph_bit_radius() <= 32


def test_null_arguments(vx):
    L = vx.lib()
    buf = np.full(4, 0x5A5A5A5A, np.uint32)
    h = ctypes.c_void_p()
    assert L.vx_grid_morph(None, 0, 1, ctypes.byref(h)) == INVALID_ARG and not h.value
    assert L.vx_grid_seal(None, 1, ctypes.byref(h)) == INVALID_ARG and not h.value
    assert L.vx_grid_morph_mask(None, 0, 1, buf.ctypes.data, 4) == INVALID_ARG
    assert L.vx_grid_morph_device(None, 0, 1, buf.ctypes.data, 4) == INVALID_ARG
    assert (buf == 0x5A5A5A5A).all()


def test_radius_argument(vx):
    assert vx.morph_radius_sq(radius=1.5) == 2 and vx.morph_radius_sq(radius=1) == 1 and vx.morph_radius_sq(radius=2.3) == 5
    assert vx.morph_radius_sq(radius_sq=14) == 14 and vx.morph_radius_sq(radius=0) == 0
    for bad in (dict(), dict(radius=1, radius_sq=1), dict(radius=-1.0), dict(radius_sq=-3), dict(radius=float("nan"))):
        with pytest.raises(ValueError):
            vx.morph_radius_sq(**bad)
