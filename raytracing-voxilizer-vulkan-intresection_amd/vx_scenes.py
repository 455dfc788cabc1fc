"""Deterministic synthetic scenes.

The reference ships no geometry (`*.obj` is git-ignored, /root/reference/.gitignore:8; media/scenes holds only
.mtl files), so every mesh named in BASELINE.json's configs is synthesised here from fixed seeds.  All generators
return (verts float32[V,3], tris int32[T,3]); `write_obj` emits `v`/`f i j k` lines with %.9g so that a float32
survives the text round trip exactly.
"""
import numpy as np


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def cube(half=1.0, center=(0.0, 0.0, 0.0)):
    """Axis-aligned cube, 8 vertices / 12 triangles (the cube.obj of BASELINE.json configs[0])."""
    c = np.array(center, dtype=np.float64)
    v = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], dtype=np.float64) * half + c
    q = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    t = []
    for a, b, c_, d in q:
        t += [(a, b, c_), (a, c_, d)]
    return _f32(v), np.array(t, dtype=np.int32)


def rotated_cube(half=1.0, angles=(0.37, 0.61, 0.23), offset=(0.113, -0.071, 0.057)):
    """Cube under a fixed non-trivial rotation + offset: no face coincides with a voxel plane."""
    v, t = cube(half)
    ax, ay, az = angles
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    r = rz @ ry @ rx
    return _f32(v.astype(np.float64) @ r.T + np.array(offset)), t


def blob(nlon=190, nlat=185, seed=1):
    """Closed lumpy lat-long sphere, 2*nlon*(nlat-1) triangles (default 69 920: the '~70k-tri bunny' stand-in)."""
    rng = np.random.default_rng(seed)
    k = rng.normal(size=(6, 3))
    ph = rng.uniform(0, 2 * np.pi, size=6)
    amp = np.array([0.22, 0.15, 0.11, 0.08, 0.06, 0.04])
    th = np.linspace(0, np.pi, nlat + 1)[1:-1]
    lo = np.linspace(0, 2 * np.pi, nlon, endpoint=False)
    T, L = np.meshgrid(th, lo, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(L), np.cos(T), np.sin(T) * np.sin(L)], axis=-1).reshape(-1, 3)
    poles = np.array([[0, 1.0, 0], [0, -1.0, 0]])
    d = np.concatenate([d, poles])
    r = 1.0 + sum(a * np.sin((d @ kk) * (2.0 + 1.5 * j) + p) for j, (a, kk, p) in enumerate(zip(amp, k, ph)))
    v = d * r[:, None] * np.array([1.0, 1.25, 0.8])
    # normalise so the bbox is exactly [-1,1]^3: voxelsize 2/256 then gives exactly 256^3 cells
    v = (v - v.min(0)) / (v.max(0) - v.min(0)) * 2.0 - 1.0
    nr = nlat - 1
    tris = []
    idx = np.arange(nr * nlon).reshape(nr, nlon)
    a = idx[:-1, :]
    b = np.roll(idx, -1, axis=1)[:-1, :]
    c = idx[1:, :]
    e = np.roll(idx, -1, axis=1)[1:, :]
    tris.append(np.stack([a, c, b], -1).reshape(-1, 3))
    tris.append(np.stack([b, c, e], -1).reshape(-1, 3))
    north, south = nr * nlon, nr * nlon + 1
    tris.append(np.stack([np.full(nlon, north), idx[0], np.roll(idx[0], -1)], -1))
    tris.append(np.stack([np.full(nlon, south), np.roll(idx[-1], -1), idx[-1]], -1))
    return _f32(v), np.concatenate(tris).astype(np.int32)


def smooth_attributes(v, t):
    """corner attributes of a closed blob-like mesh: smooth normals (the area-weighted vertex normals, float64, unit) and spherical uvs
    (u = 0.5 + atan2(z, x) / 2pi, v = acos(y) / pi of the direction from the centre) -> (normals [T, 3, 3], uvs [T, 3, 2]) float32"""
    v64 = np.asarray(v, np.float64)
    t = np.asarray(t, np.int64)
    p = v64[t]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    vn = np.zeros_like(v64)
    for k in range(3):
        np.add.at(vn, t[:, k], fn)
    vn /= np.maximum(np.linalg.norm(vn, axis=1, keepdims=True), 1e-30)
    c = v64 - 0.5 * (v64.min(0) + v64.max(0))
    d = c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-30)
    uv = np.stack([0.5 + np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi), np.arccos(np.clip(d[:, 1], -1.0, 1.0)) / np.pi], 1)
    return _f32(vn[t]), _f32(uv[t])


def checker_texture(w, h, cells=8, seed=0):
    """an RGBA8 checker of w x h texels (top row first), cells x cells squares of two random colours with a gradient over them"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, 3), rng.integers(0, 256, 3)
    y, x = np.mgrid[0:h, 0:w]
    on = ((x * cells // w) + (y * cells // h)) % 2 == 1
    rgb = np.where(on[..., None], a, b).astype(np.int64)
    rgb = (rgb * (128 + (x * 127 // max(w - 1, 1)))[..., None]) // 255
    return np.concatenate([rgb.astype(np.uint8), np.full((h, w, 1), 255, np.uint8)], 2)


def attr_blob_field(n=32, tex=1024):
    """the blob-instance field of attribute shading's timings: a 5.9k-triangle blob with smooth corner normals and spherical uvs into a
    tex x tex checker, placed n x n times at scale 0.3 on a 0.75 pitch (x, z from -12, y = 1) -> dict(verts, tris, normals, uvs, texture,
    transforms [n*n, 12] row-major object-to-world)"""
    v, t = blob(nlon=60, nlat=50)
    nrm, uv = smooth_attributes(v, t)
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    tr = np.zeros((n * n, 12), np.float32)
    tr[:, 0] = tr[:, 5] = tr[:, 10] = 0.3
    tr[:, 3] = -12 + g[:, 0] * 0.75
    tr[:, 7] = 1.0
    tr[:, 11] = -12 + g[:, 1] * 0.75
    return dict(verts=v, tris=t, normals=nrm, uvs=uv, texture=checker_texture(tex, tex, cells=16, seed=5), transforms=tr)


def _grid_sheet(p00, du, dv, nu, nv, disp=None):
    u = np.linspace(0, 1, nu + 1)
    w = np.linspace(0, 1, nv + 1)
    U, W = np.meshgrid(u, w, indexing="ij")
    p = np.array(p00)[None, None, :] + U[..., None] * np.array(du) + W[..., None] * np.array(dv)
    if disp is not None:
        p = p + disp(U, W)
    idx = np.arange((nu + 1) * (nv + 1)).reshape(nu + 1, nv + 1)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    t = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return p.reshape(-1, 3), t


def _cylinder(base, radius, height, nseg, nrings, flute=0.0):
    ang = np.linspace(0, 2 * np.pi, nseg, endpoint=False)
    hs = np.linspace(0, height, nrings + 1)
    A, Hh = np.meshgrid(ang, hs, indexing="ij")
    r = radius * (1.0 + flute * np.cos(12 * A))
    p = np.stack([base[0] + r * np.cos(A), base[1] + Hh, base[2] + r * np.sin(A)], -1)
    idx = np.arange(nseg * (nrings + 1)).reshape(nseg, nrings + 1)
    a, b = idx[:, :-1], np.roll(idx, -1, axis=0)[:, :-1]
    c, d = np.roll(idx, -1, axis=0)[:, 1:], idx[:, 1:]
    t = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return p.reshape(-1, 3), t


def atrium(seed=3, detail=1.0):
    """Sponza-like architectural hall (default ~262k triangles, bbox exactly [-16,16]x[0,32]x[-16,16]): a floor, walls and a ceiling made of a few LARGE
    triangles, two colonnades of fluted columns, arches between them and hanging drapes (finely tessellated
    displaced sheets).  Mixes candidate boxes of 10^1 and 10^7 voxels, which is what stresses the voxelizer's
    load balancing at 512^3 / 1024^3."""
    rng = np.random.default_rng(seed)
    parts = []

    def add(p, t):
        parts.append((np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.int64)))

    Lx, Ly, Lz = 32.0, 32.0, 32.0   # bbox exactly 32^3: voxelsize 32/512 gives exactly 512^3 cells
    # big flat surfaces: 2 triangles each, deliberately NOT on round coordinates
    add(*_grid_sheet((-Lx / 2, 0.013, -Lz / 2), (Lx, 0, 0), (0, 0, Lz), 1, 1))            # floor
    add(*_grid_sheet((-Lx / 2, Ly - 0.021, -Lz / 2), (Lx, 0, 0), (0, 0, Lz), 1, 1))       # ceiling
    add(*_grid_sheet((-Lx / 2, 0, -Lz / 2 + 0.017), (Lx, 0, 0), (0, Ly, 0), 1, 1))        # back wall
    add(*_grid_sheet((-Lx / 2 + 0.011, 0, -Lz / 2), (0, 0, Lz), (0, Ly, 0), 1, 1))        # left wall
    add(*_grid_sheet((Lx / 2 - 0.019, 0, -Lz / 2), (0, 0, Lz), (0, Ly, 0), 1, 1))         # right wall
    # slanted roof beams: large diagonal triangles
    for k in range(6):
        x0 = -Lx / 2 + (k + 0.5) * Lx / 6
        add(np.array([[x0, Ly * 0.7, -Lz / 2], [x0 + 0.8, Ly * 0.98, 0.1], [x0 - 0.3, Ly * 0.72, Lz / 2]]), np.array([[0, 1, 2]]))
    ncol = 12
    nseg, nrings = int(48 * detail), int(48 * detail)
    for side in (-1, 1):
        for k in range(ncol):
            x = -Lx / 2 + (k + 0.5) * Lx / ncol + rng.uniform(-0.05, 0.05)
            z = side * Lz * 0.27
            add(*_cylinder((x, 0.0, z), 0.62, Ly * 0.55, nseg, nrings, flute=0.04))
            # capital: a squat wider cylinder
            add(*_cylinder((x, Ly * 0.55, z), 0.85, 0.5, nseg, 2))
    # arches between neighbouring columns
    na = int(40 * detail)
    for side in (-1, 1):
        for k in range(ncol - 1):
            x0 = -Lx / 2 + (k + 0.5) * Lx / ncol
            x1 = x0 + Lx / ncol
            z = side * Lz * 0.27

            def arch(U, W, x0=x0, x1=x1):
                th = np.pi * U
                return np.stack([0 * U, 1.1 * np.sin(th), 0 * U], -1)
            add(*_grid_sheet((x0, Ly * 0.55 + 0.5, z - 0.3), (x1 - x0, 0, 0), (0, 0, 0.6), na, 4, arch))
    # drapes: finely tessellated wavy sheets
    nd = int(118 * detail)
    for k in range(5):
        x0 = -Lx / 2 + 2.0 + k * 6.0
        ph = rng.uniform(0, 6.28)

        def wave(U, W, ph=ph):
            return np.stack([0.0 * U, 0.25 * np.sin(5 * U * np.pi + ph) * W, 0.35 * np.sin(9 * U * np.pi + ph) * (0.3 + W)], -1)
        add(*_grid_sheet((x0, Ly * 0.9, -1.0), (3.6, 0, 0), (0, -Ly * 0.5, 0.4), nd, nd, wave))
    vs, ts, off = [], [], 0
    for p, t in parts:
        vs.append(p)
        ts.append(t + off)
        off += p.shape[0]
    return _f32(np.concatenate(vs)), np.concatenate(ts).astype(np.int32)


def soup(ntri, seed=4, edge=0.004, extent=1.0):
    """Random small triangles: centres uniform in [0,extent]^3, vertices within +-edge of the centre.  Vertices are
    not shared (V = 3T).  C5's 10M-triangle soup is soup(10_000_000, 4, edge=1.5/2048)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, extent, size=(ntri, 1, 3))
    v = c + rng.uniform(-edge, edge, size=(ntri, 3, 3))
    v = np.clip(v, 0.0, extent)
    return _f32(v.reshape(-1, 3)), np.arange(3 * ntri, dtype=np.int32).reshape(-1, 3)


def adversarial(seed=7):
    """Knife-edge inputs: walls exactly on multiples of 0.125, zero-area / collinear /
    repeated-vertex triangles, edges <= 1e-9, bbox-spanning diagonal triangles, grid-snapped small triangles."""
    rng = np.random.default_rng(seed)
    V, T = [], []

    def tri(a, b, c):
        n = len(V)
        V.extend([a, b, c])
        T.append((n, n + 1, n + 2))
    for k in range(9):
        x = k * 0.125
        tri((x, 0, 0), (x, 1, 0), (x, 1, 1))
        tri((0, x, 0), (1, x, 0), (1, x, 1))
        tri((0, 0, x), (1, 0, x), (1, 1, x))
    for _ in range(60):
        p = rng.uniform(0, 1, 3)
        q = rng.uniform(0, 1, 3)
        tri(p, p, p)                       # point
        tri(p, q, p)                       # repeated vertex
        tri(p, (p + q) / 2, q)             # collinear
        tri(p, p + 1e-9, p + np.array([0, 1e-9, 0]))  # tiny
    for _ in range(50):
        a = rng.integers(0, 2, 3).astype(float)
        tri(a, 1 - a, rng.uniform(0, 1, 3))  # spans the bbox diagonally
    g = rng.integers(0, 64, size=(2000, 3)) / 64.0
    for p in g:
        d = rng.integers(-2, 3, size=(2, 3)) / 64.0
        tri(p, np.clip(p + d[0], 0, 1), np.clip(p + d[1], 0, 1))
    return _f32(np.array(V)), np.array(T, dtype=np.int32)


def random_rays(n, bmin, bmax, seed=2):
    """origins uniform on a sphere of radius 2x the bbox diagonal around the bbox centre,
    directions toward uniform points inside the bbox (not normalised away from unit length: they ARE normalised).
    No zero direction components (0*inf would give NaN in the slab formula)."""
    rng = np.random.default_rng(seed)
    bmin = np.asarray(bmin, np.float64)
    bmax = np.asarray(bmax, np.float64)
    ctr = (bmin + bmax) / 2
    R = 2.0 * np.linalg.norm(bmax - bmin)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = ctr + R * d
    tgt = rng.uniform(bmin, bmax, size=(n, 3))
    dr = tgt - o
    dr /= np.linalg.norm(dr, axis=1, keepdims=True)
    dr = dr.astype(np.float32)
    dr[dr == 0] = np.float32(1e-20)
    return np.ascontiguousarray(np.concatenate([o.astype(np.float32), dr], axis=1))


def camera_matrices(eye=(6.16636, 2.42256, -3.15471), ctr=(0.0, 1.0, 0.0), up=(0.0, 1.0, 0.0), fov_deg=60.0,
                    aspect=1280.0 / 720.0, near=0.1, far=1000.0):
    """viewInverse / projInverse as the reference uploads them (hello_vulkan.cpp:69-77; camera main.cpp:92):
    lookAt RH, perspectiveRH_ZO with [1][1] *= -1.  Column-major float32[16] each.  The fov is nvpro_core's
    CameraManip default, third-party and not in the tree (believed 60 deg; unpinned)."""
    eye, ctr, up = (np.array(a, np.float64) for a in (eye, ctr, up))
    f = ctr - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = s, u, -f
    view[:3, 3] = [-s @ eye, -u @ eye, f @ eye]
    t = np.tan(np.radians(fov_deg) / 2)
    proj = np.zeros((4, 4))
    proj[0, 0] = 1 / (aspect * t)
    proj[1, 1] = -1 / t
    proj[2, 2] = far / (near - far)
    proj[3, 2] = -1
    proj[2, 3] = -(far * near) / (far - near)
    vi = np.linalg.inv(view).T.astype(np.float32).reshape(16)   # .T -> column-major
    pi = np.linalg.inv(proj).T.astype(np.float32).reshape(16)
    return vi, pi


# Cameras INSIDE the atrium hall (bbox [-16,16] x [0,32] x [-16,16], open towards +z): what the reference renders -- its camera stands in
# the scene (main.cpp:92) -- as opposed to bench.py's headline batch, whose rays start outside a scene closed on five sides.
INTERIOR_CAMERAS = (dict(eye=(0.0, 6.0, 14.0), ctr=(-2.0, 10.0, -16.0)), dict(eye=(-10.0, 12.0, 10.0), ctr=(8.0, 8.0, -12.0)))


# ---- closed meshes for solid voxelization (VX_VOXELIZE_SOLID) ----
def _rotate(v, angles=(0.37, 0.61, 0.23), offset=(0.113, -0.071, 0.057)):
    ax, ay, az = angles
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    return np.asarray(v, dtype=np.float64) @ (rz @ ry @ rx).T + np.array(offset)


def torus(major=1.0, minor=0.38, nu=96, nv=48):
    """Closed torus around the y axis: its tube is filled by a solid build, the hole through the middle stays empty."""
    u = np.linspace(0, 2 * np.pi, nu, endpoint=False)
    w = np.linspace(0, 2 * np.pi, nv, endpoint=False)
    U, W = np.meshgrid(u, w, indexing="ij")
    r = major + minor * np.cos(W)
    v = np.stack([r * np.cos(U), minor * np.sin(W), r * np.sin(U)], -1).reshape(-1, 3)
    i = np.arange(nu)[:, None]
    j = np.arange(nv)[None, :]
    a = i * nv + j
    b = ((i + 1) % nu) * nv + j
    c = ((i + 1) % nu) * nv + (j + 1) % nv
    d = i * nv + (j + 1) % nv
    t = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return _f32(_rotate(v, (0.21, 0.13, 0.05), (0.0, 0.0, 0.0))), t.astype(np.int32)


def nested_shells(outer=1.0, inner=0.45):
    """Two closed shells, one inside the other (a rotated cube around a smaller one): a solid build fills both and the gap between them."""
    v0, t0 = cube(outer)
    v1, t1 = cube(inner, center=(0.05, -0.03, 0.02))
    v = np.concatenate([v0, v1]).astype(np.float64)
    return _f32(_rotate(v)), np.concatenate([t0, t1 + v0.shape[0]]).astype(np.int32)


def holed_box(hole, half=1.0):
    """A closed box whose +z face has a square hole of side `hole` at its centre (the face is the four rectangles around it), rotated so that
    no face lies in a voxel plane.  A hole several voxels wide lets the exterior in (no interior); one narrower than a voxel is closed by the
    conservative surface (the box is filled)."""
    h, k = half, hole / 2.0
    corners = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], dtype=np.float64) * h
    tris = []
    verts = [c for c in corners]
    q = [(0, 2, 3, 1), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]  # every face of cube() but +z
    for a, b, c, d in q:
        tris += [(a, b, c), (a, c, d)]

    def quad(p0, p1, p2, p3):
        n = len(verts)
        verts.extend([np.array(p, dtype=np.float64) for p in (p0, p1, p2, p3)])
        tris.extend([(n, n + 1, n + 2), (n, n + 2, n + 3)])
    z = h
    quad((-h, -h, z), (h, -h, z), (h, -k, z), (-h, -k, z))   # below the hole
    quad((-h, k, z), (h, k, z), (h, h, z), (-h, h, z))       # above it
    quad((-h, -k, z), (-k, -k, z), (-k, k, z), (-h, k, z))   # left of it
    quad((k, -k, z), (h, -k, z), (h, k, z), (k, k, z))       # right of it
    return _f32(_rotate(np.array(verts))), np.array(tris, dtype=np.int32)


def spiral_maze(n=96, closed_core=True):
    """A bitmask (bool[Z, Y, X], n^3) of nested cubic shells one cell thick with a one-cell gap between them.  Shell k has a single opening at the
    centre of its +x face (k even) or -x face (k odd), so the way in from the boundary winds half around every shell: at least three turns per
    shell.  With closed_core the innermost shell has no opening and its inside is the interior."""
    m = np.zeros((n, n, n), dtype=bool)
    c = n // 2
    shells = []
    lo = 1
    while n - 1 - lo - lo >= 4:
        shells.append(lo)
        lo += 2
    for k, lo in enumerate(shells):
        hi = n - 1 - lo
        m[lo:hi + 1, lo:hi + 1, lo] = m[lo:hi + 1, lo:hi + 1, hi] = True
        m[lo:hi + 1, lo, lo:hi + 1] = m[lo:hi + 1, hi, lo:hi + 1] = True
        m[lo, lo:hi + 1, lo:hi + 1] = m[hi, lo:hi + 1, lo:hi + 1] = True
        if not (closed_core and k == len(shells) - 1):
            m[c, c, hi if k % 2 == 0 else lo] = False
    return m

def write_obj(path, verts, tris, header="synthetic scene"):
    v = np.asarray(verts, dtype=np.float32)
    t = np.asarray(tris, dtype=np.int64) + 1
    with open(path, "w") as fh:
        fh.write("# %s\n" % header)
        fh.write("".join("v %.9g %.9g %.9g\n" % (a, b, c) for a, b, c in v.tolist()))
        fh.write("".join("f %d %d %d\n" % (a, b, c) for a, b, c in t.tolist()))


def scene(name):
    """Named scenes used by bench.py / tests / the CLI fixtures."""
    if name == "cube":
        return cube()
    if name == "rotcube":
        return rotated_cube()
    if name == "blob70k":
        return blob()
    if name == "atrium262k":
        return atrium()
    if name == "adversarial":
        return adversarial()
    if name.startswith("soup"):
        n = int(name[4:].replace("k", "000").replace("m", "000000"))
        return soup(n)
    raise KeyError(name)
