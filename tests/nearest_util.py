"""helpers of the nearest-hit library's tests (test_nearest_statement.py, test_gpu_nearest*.py): nearest_np, the float32 numpy
statement of rls_nearest_hits (include/rlshaders_amd_nearest.h) -- every triangle against every ray, no tree --, a float64 brute
force to hold it to, hits_at (the statement at one given triangle per ray: the planes of a brute force's (prim, t)), the meshes
(icosphere, quad grid, triangle soup, the rules' mesh; the deep ones: deep_grid, two_sheets, mid_soup, copies, huge_soup) and the
hostile and the stack-filling ray streams shared by the CPU and the GPU tests, and numpy tracers over the statement in the shape
the walks' numpy statements take.  pytest does not collect this module."""
import numpy as np

F = np.float32
NO_PRIM = 0xFFFFFFFF
MAX_TRIANGLES = 1 << 22
STACK = 24


class Mesh:
    """V float32 [nv, 3], tri uint32 [nt, 3], surface uint32 [nt] or None, normals float32 [nv, 3] or None"""

    def __init__(self, V, tri, surface=None, normals=None):
        self.V = np.ascontiguousarray(V, F).reshape(-1, 3)
        self.tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
        self.surface = None if surface is None else np.ascontiguousarray(surface, np.uint32)
        self.normals = None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3)

    @property
    def nt(self):
        return self.tri.shape[0]


# ---- the statement -----------------------------------------------------------------------------------------------------------------
def _min(a, b):
    return np.where(b < a, b, a)


def _max(a, b):
    return np.where(b > a, b, a)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _normalize(a):
    l = np.sqrt(_dot(a, a))
    return np.stack([a[0] / l, a[1] / l, a[2] / l]).astype(F)


class Hits:
    """hit uint8 [M], t, u, v float32 [M], prim, surface uint32 [M], P, N, Ns, T, wo float32 [3, M]; entries without a hit hold 0"""


def _candidate(v0, v1, v2, o, d, inv, sign):
    """The statement's box interval and triangle test of one triangle per ray -> (box, tri_hit, t, u, v), each [M].  v0, v1, v2:
    the triangle's vertices by component -- v[c] a float32 scalar (one triangle against every ray, nearest_np) or a float32
    array [M] (a triangle of its own per ray, hits_at): the same float32 operations in the same order either way."""
    M = o.shape[1]
    lo, hi = [_min(_min(v0[c], v1[c]), v2[c]) for c in range(3)], [_max(_max(v0[c], v1[c]), v2[c]) for c in range(3)]
    tn, tf = np.zeros(M, F), np.full(M, np.inf, F)
    for c in range(3):
        a, b = (lo[c] - o[c]) * inv[c], (hi[c] - o[c]) * inv[c]
        a, b = np.where(sign[c], b, a), np.where(sign[c], a, b)
        tn = np.where(a > tn, a, tn)
        tf = np.where(b < tf, b, tf)
    box = ~(tn > tf)
    e1, e2 = [v1[c] - v0[c] for c in range(3)], [v2[c] - v0[c] for c in range(3)]
    p = _cross(d, e2)
    det = _dot(e1, p)
    r = F(1) / det
    s = [o[0] - v0[0], o[1] - v0[1], o[2] - v0[2]]
    u = _dot(s, p) * r
    q = _cross(s, e1)
    v = _dot(d, q) * r
    tm = _dot(e2, q) * r
    tri_hit = ((det < 0) | (det > 0)) & (u >= 0) & (v >= 0) & (u + v <= F(1)) & ~np.isnan(tm)
    t = tm
    t = np.where(tn > t, tn, t)
    t = np.where(tf < t, tf, t)
    return box, tri_hit, t, u, v


def _report(mesh, o, d, hit, prim, best_t, best_u, best_v):
    """what a hit reports, from the winner's (prim, t, u, v): the statement's P, surface, N, Ns, T, wo; 0 where hit is unset"""
    M = o.shape[1]
    V = mesh.V
    h = Hits()
    prim = np.where(hit, prim, 0)
    h.hit, h.prim = hit.astype(np.uint8), prim.astype(np.uint32)
    h.t, h.u, h.v = best_t.astype(F), best_u.astype(F), best_v.astype(F)
    h.surface = np.zeros(M, np.uint32) if mesh.surface is None or mesh.nt == 0 else np.where(hit, mesh.surface[prim], 0).astype(np.uint32)
    h.P = np.stack([o[c] + h.t * d[c] for c in range(3)]).astype(F)
    h.wo = (-d).astype(F)
    if mesh.nt:
        ix = mesh.tri[prim].astype(np.int64)
        v0, v1, v2 = (V[ix[:, k]].T for k in range(3))
        e1, e2 = v1 - v0, v2 - v0
        h.N = _normalize(_cross(e1, e2))
        h.T = _normalize(e1)
        if mesh.normals is None:
            h.Ns = h.N.copy()
        else:
            n0, n1, n2 = (mesh.normals[ix[:, k]].T for k in range(3))
            w = (F(1) - h.u) - h.v
            h.Ns = _normalize([(w * n0[c] + h.u * n1[c]) + h.v * n2[c] for c in range(3)])
    else:
        h.N, h.Ns, h.T = np.zeros((3, M), F), np.zeros((3, M), F), np.zeros((3, M), F)
    for name in ("P", "N", "Ns", "T", "wo"):
        setattr(h, name, np.where(hit, getattr(h, name), F(0)).astype(F))
    return h


def _ray_args(o, d, m, skip):
    o, d = np.asarray(o, F), np.asarray(d, F)
    M = o.shape[1]
    m = np.full(M, np.inf, F) if m is None else np.asarray(m, F)
    skip = np.full(M, NO_PRIM, np.int64) if skip is None else np.asarray(skip).astype(np.int64) & 0xFFFFFFFF
    return o, d, M, m, skip


def nearest_np(mesh, o, d, m=None, skip=None):
    """The statement: o, d float32 [3, M]; m float32 [M] or None (+inf); skip uint32 [M] or None (nothing).  Every operation is
    a float32 numpy operation, rounded by itself."""
    o, d, M, m, skip = _ray_args(o, d, m, skip)
    best_t, best_u, best_v = np.zeros(M, F), np.zeros(M, F), np.zeros(M, F)
    best = np.full(M, -1, np.int64)
    V = mesh.V
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(F)
        sign = np.signbit(inv)
        for i in range(mesh.nt):
            v0, v1, v2 = (V[int(k)] for k in mesh.tri[i])
            box, tri_hit, t, u, v = _candidate(v0, v1, v2, o, d, inv, sign)
            cand = (skip != i) & box & tri_hit & (t > 0) & (t <= m)
            take = cand & ((best < 0) | (t < best_t))                # ascending i: a tie keeps the smaller index
            best_t, best_u, best_v = np.where(take, t, best_t), np.where(take, u, best_u), np.where(take, v, best_v)
            best = np.where(take, i, best)
        return _report(mesh, o, d, best >= 0, best, best_t, best_u, best_v)


def hits_at(mesh, o, d, prim, m=None, skip=None):
    """The statement's candidate rule at ONE given triangle per ray, prim uint32 [M] (NO_PRIM: none), vectorised over the rays:
    hit is set where that triangle is a candidate of its ray, and t, u, v and every reported plane are what nearest_np gives
    where that triangle is the winner -- _candidate and _report are the body of nearest_np.  It turns the (prim, t) of a brute
    force over a mesh too large for nearest_np's loop (tests/native/nearest_host_check.cpp, file mode) into all the planes, and
    ties that program's restatement to this one: the t recomputed here must equal its t bit for bit."""
    o, d, M, m, skip = _ray_args(o, d, m, skip)
    prim = np.asarray(prim).astype(np.int64) & 0xFFFFFFFF
    given = prim != NO_PRIM
    at = np.where(given, prim, 0)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(F)
        sign = np.signbit(inv)
        if mesh.nt == 0:
            return _report(mesh, o, d, np.zeros(M, bool), at, np.zeros(M, F), np.zeros(M, F), np.zeros(M, F))
        ix = mesh.tri[at].astype(np.int64)
        v0, v1, v2 = (np.ascontiguousarray(mesh.V[ix[:, k]].T) for k in range(3))
        box, tri_hit, t, u, v = _candidate(v0, v1, v2, o, d, inv, sign)
        cand = given & (skip != prim) & box & tri_hit & (t > 0) & (t <= m)
        z = np.zeros(M, F)
        return _report(mesh, o, d, cand, at, np.where(cand, t, z), np.where(cand, u, z), np.where(cand, v, z))


def brute64(mesh, o, d, m=None):
    """Moller-Trumbore in float64 over every triangle, no boxes -> (hit, prim, t, margin): margin [M] is the smallest of
    u, v, 1 - u - v at the winner and the gap to the runner-up's t (how far the ray is from an edge or another surface)"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    M = o.shape[1]
    m = np.full(M, np.inf) if m is None else np.asarray(m, np.float64)
    V = mesh.V.astype(np.float64)
    v0, v1, v2 = (V[mesh.tri[:, k].astype(np.int64)] for k in range(3))          # [nt, 3]
    e1, e2 = v1 - v0, v2 - v0
    with np.errstate(all="ignore"):
        p = np.cross(d.T[None, :, :], e2[:, None, :])                             # [nt, M, 3]
        det = np.einsum("tc,tmc->tm", e1, p)
        s = o.T[None, :, :] - v0[:, None, :]
        u = np.einsum("tmc,tmc->tm", s, p) / det
        q = np.cross(s, e1[:, None, :])
        v = np.einsum("mc,tmc->tm", d.T, q) / det
        t = np.einsum("tc,tmc->tm", e2, q) / det
        edge = np.minimum(np.minimum(u, v), 1 - u - v)
        ok = (det != 0) & (edge >= 0) & (t > 0) & (t <= m[None, :])
        # a near miss counts against the margin too: a ray that passes a triangle's edge closely on the outside
        near_miss = np.where((det != 0) & (t > 0) & (t <= m[None, :]) & ~ok, -edge, np.inf).min(axis=0, initial=np.inf)
        tt = np.where(ok, t, np.inf)
        k = np.argmin(tt, axis=0) if mesh.nt else np.zeros(M, np.int64)
        at = np.arange(M)
        best = tt[k, at] if mesh.nt else np.full(M, np.inf)
        hit = np.isfinite(best)
        tt2 = tt.copy()
        if mesh.nt:
            tt2[k, at] = np.inf
        gap = (tt2.min(axis=0, initial=np.inf) - best) if mesh.nt else np.full(M, np.inf)
        margin = np.minimum(np.where(hit, np.minimum(edge[k, at] if mesh.nt else np.inf, gap), np.inf), near_miss)
    return hit, k, np.where(hit, best, 0.0), margin


# ---- the meshes ----------------------------------------------------------------------------------------------------------------
def icosphere(level=2, radius=1.0, center=(0.0, 0.0, 0.0), surface=0):
    """a subdivided icosahedron: 20 * 4^level triangles, outward facing, per-vertex normals = the unit positions"""
    g = (1 + 5 ** 0.5) / 2
    V = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    V = [np.array(v, np.float64) / np.linalg.norm(v) for v in V]
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, T2 = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                w = V[a] + V[b]
                V.append(w / np.linalg.norm(w))
                mid[key] = len(V) - 1
            return mid[key]

        for a, b, c in T:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            T2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        T = T2
    unit = np.array(V)
    return Mesh(unit * radius + np.asarray(center, np.float64), T, surface=np.full(len(T), surface, np.uint32), normals=unit)


def quad_grid(n=33, surfaces=5, flat=False):
    """n x n quads over [-1, 1]^2, two triangles each, on a gently bumped height field (flat: in the plane z = 0); surface = quad
    index % surfaces"""
    g = np.linspace(-1.0, 1.0, n + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    z = 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y) * (0.0 if flat else 1.0)
    V = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    j, i = np.divmod(np.arange(n * n, dtype=np.int64), n)           # quad q = j * n + i: triangles 2 q (under the diagonal), 2 q + 1
    a = j * (n + 1) + i
    T = np.stack([a, a + 1, a + n + 2, a, a + n + 2, a + n + 1], axis=1).reshape(-1, 3)
    S = np.repeat((j * n + i) % surfaces, 2)
    return Mesh(V, T, surface=S)


def soup(nt=1025, seed=5):
    """random small triangles in [-1, 1]^3; every 16th is degenerate: a repeated vertex index, three collinear vertices, or a
    vertex duplicated under another index; surfaces 0 .. 299 (past any table of the tests)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (nt, 1, 3))
    V = (c + rng.uniform(-0.2, 0.2, (nt, 3, 3))).astype(F)
    tri = np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3)
    for i in range(0, nt, 16):
        kind = (i // 16) % 3
        if kind == 0:
            tri[i, 2] = tri[i, 1]
        elif kind == 1:
            V[i, 2] = V[i, 0] + (V[i, 1] - V[i, 0]) * F(2)
        else:
            V[i, 2] = V[i, 1]
    return Mesh(V.reshape(-1, 3), tri, surface=rng.integers(0, 300, nt), normals=rng.normal(size=(3 * nt, 3)))


def single_triangle():
    return Mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 2)], surface=[3])


def empty_mesh():
    return Mesh(np.zeros((3, 3), F), np.zeros((0, 3), np.uint32))


def rules_mesh():
    """the mesh the rule streams run on: the unit square at z = 0 as two triangles sharing the diagonal (0, 1), both again as
    (2, 3) -- coincident, so every hit ties --, a square at z = 1 (4, 5), a flat triangle in the plane x = 2 (6), a triangle with
    a repeated index (7), three collinear vertices (8), a vertex duplicated under another index (9, the same points as 0)"""
    V = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0),                 # 0 .. 3
         (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1),                 # 4 .. 7
         (2, 0, 0), (2, 1, 0), (2, 0, 1),                            # 8 .. 10
         (0.25, 0.25, 0.5), (0.75, 0.25, 0.5), (0.5, 0.25, 0.5),     # 11 .. 13: collinear
         (0, 0, 0)]                                                  # 14: vertex 0 again
    T = [(0, 1, 2), (0, 2, 3), (0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7), (8, 9, 10), (11, 12, 12), (11, 12, 13), (14, 1, 2)]
    return Mesh(V, T, surface=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9])


# ---- deep meshes: trees whose depth reaches what the traversal stack is sized for (test_nearest_deep.py, test_gpu_nearest_deep.py)
DEEP_N = 1024               # quads a side of the deep grid: 1025 vertices a side, cells of 2 / 1024, 2^21 triangles
DEEP_EXTRA = 20


def deep_grid():
    """A DEEP_N x DEEP_N height field (heights within 1e-4, far below the cell size, so that no split of it is along z), plus
    DEEP_EXTRA small triangles at z = 1 over the cells around (0.55, 0.55) with surface ids of their own, and per-vertex normals:
    nt = 2^21 + 20, a tree of 23 levels at leaf_size 1 and of 20 at leaf_size 8.  Triangle 0 has the smallest centroid in x and
    in y: it lies in the left (larger) half of every split, in a deepest leaf."""
    rng = np.random.default_rng(77)
    g = quad_grid(DEEP_N, flat=True)
    V = g.V.astype(np.float64)
    V[:, 2] = rng.uniform(-1e-4, 1e-4, V.shape[0])
    k = np.arange(DEEP_EXTRA)
    c = np.stack([0.55 + 0.01 * (k % 5), 0.55 + 0.01 * (k // 5), np.ones(DEEP_EXTRA)], axis=1)
    extra = c[:, None, :] + np.array([(-0.003, -0.002, 0.0), (0.003, -0.002, 0.0), (0.0, 0.004, 0.0)])[None]
    nv = V.shape[0]
    tri = np.concatenate([g.tri, (nv + np.arange(3 * DEEP_EXTRA, dtype=np.uint32)).reshape(-1, 3)])
    V = np.concatenate([V, extra.reshape(-1, 3)])
    normals = np.concatenate([rng.uniform(-0.2, 0.2, (V.shape[0], 2)), np.ones((V.shape[0], 1))], axis=1)
    mesh = Mesh(V, tri, surface=np.concatenate([g.surface, 1000 + k]), normals=normals)
    assert mesh.nt == (1 << 21) + DEEP_EXTRA
    return mesh


def two_sheets():
    """the documented limit itself, RLS_NEAREST_MAX_TRIANGLES = 2^22 triangles: two DEEP_N x DEEP_N sheets, at z about 0 and 0.5"""
    g = deep_grid()
    nv, nt = (DEEP_N + 1) ** 2, 1 << 21
    V = np.concatenate([g.V[:nv], g.V[:nv] + F([0.0, 0.0, 0.5])])
    tri = np.concatenate([g.tri[:nt], g.tri[:nt] + np.uint32(nv)])
    mesh = Mesh(V, tri, surface=np.concatenate([g.surface[:nt], g.surface[:nt] + 5]))
    assert mesh.nt == MAX_TRIANGLES
    return mesh


def mid_soup():
    """the soup at 2^17 + 1 triangles: 19 levels at leaf_size 1"""
    return soup((1 << 17) + 1, seed=8)


def copies(K=4097):
    """K triangles over the same three vertices: every box is the same box, every hit ties, and a ray through the interior
    opens every node of the tree"""
    return Mesh([(0, 0, 0), (1, 0, 0.25), (0, 1, 0.5)], np.tile(np.array([(0, 1, 2)], np.uint32), (K, 1)), surface=np.arange(K) % 7,
                normals=[(0, 0.1, 1), (0.1, 0, 1), (-0.1, -0.1, 1)])


def huge_soup():
    """the 1025-triangle soup with every 8th triangle (3, 11, ..) shrunk to subnormal size -- edges about 1e-40; float32 holds
    such an edge only about the origin, so the triangle's first vertex is moved there -- and, of every 8th vertex, one coordinate
    scaled into [1e37, 3e38] with either sign: the builder's centroid keys lo + hi then reach +-inf and their extent NaN"""
    s = soup(1025)
    rng = np.random.default_rng(31)
    V = s.V.reshape(-1, 3, 3).copy()                                 # (a soup triangle's vertices are its own)
    for i in range(3, s.nt, 8):
        e = (V[i] - V[i, 0]).astype(np.float64) * 2.5e-40
        V[i] = (e + rng.uniform(-1e-40, 1e-40, 3)).astype(F)
    V = V.reshape(-1, 3)
    for k in range(0, V.shape[0], 8):
        V[k, (k // 8) % 3] = F(10.0 ** rng.uniform(37.0, 38.47) * (1 if rng.random() < 0.5 else -1))
    assert np.isfinite(V).all() and np.abs(V).max() > 1e38 and ((V != 0) & (np.abs(V) < 1e-38)).sum() > 500
    return Mesh(V, s.tri, surface=s.surface, normals=s.normals)


DEEP_MESHES = dict(deep_grid=deep_grid, two_sheets=two_sheets, mid_soup=mid_soup, copies=copies, huge_soup=huge_soup)


# ---- rays ------------------------------------------------------------------------------------------------------------------------
def rays_at_targets(rng, targets, spread=3.0):
    """rays from random origins at distance ~spread towards the target points [K, 3] -> o, d [3, K] (d not normalised)"""
    K = targets.shape[0]
    w = rng.normal(size=(K, 3))
    o = targets + spread * w / np.linalg.norm(w, axis=1, keepdims=True)
    d = (targets - o) * rng.uniform(0.5, 2.0, (K, 1))
    return np.ascontiguousarray(o.T, F), np.ascontiguousarray(d.T, F)


def interior_targets(rng, mesh, K, margin=0.05):
    """K points inside random triangles, barycentrics at least `margin` from every edge"""
    i = rng.integers(0, mesh.nt, K)
    b = rng.dirichlet((1, 1, 1), K) * (1 - 3 * margin) + margin
    P = mesh.V.astype(np.float64)[mesh.tri[i].astype(np.int64)]                   # [K, 3, 3]
    return np.einsum("kv,kvc->kc", b, P)


def random_rays(rng, M, box=1.5):
    """origins in a cube, directions to points of a smaller cube: a mix of hits, grazes and misses"""
    o = rng.uniform(-box, box, (3, M))
    d = rng.uniform(-1, 1, (3, M)) - o
    return o.astype(F), d.astype(F)


def _rays(rows):
    """[(o, d, m, skip)] -> o, d [3, M], m [M], skip uint32 [M]"""
    o = np.array([r[0] for r in rows], F).T
    d = np.array([r[1] for r in rows], F).T
    m = np.array([r[2] for r in rows], F)
    skip = np.array([r[3] for r in rows], np.int64).astype(np.uint32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), m, skip


def rule_streams():
    """name -> (o, d, m, skip) on rules_mesh(), each made for one rule of the statement"""
    nan, inf, none = np.nan, np.inf, NO_PRIM
    one = F(1)
    down = (0.0, 0.0, -1.0)
    s = {}
    # the shared diagonal x == y, the shared vertices, the outer edges and corners: ties go to the smaller index
    s["ties"] = _rays([((x, y, 0.5), down, inf, none) for x, y in
                       ((0.5, 0.5), (0.25, 0.25), (0, 0), (1, 1), (1, 0), (0, 1), (0.5, 0), (1, 0.5), (0.5, 1), (0, 0.5), (0.75, 0.25),
                        (0.25, 0.75))])
    # skip: the coincident copies take over one by one; a skip of a triangle not on the ray, and past the mesh, changes nothing
    s["skip"] = _rays([((0.75, 0.25, 0.5), down, inf, k) for k in (none, 0, 2, 9, 1, 7, 10, 1 << 31)] +
                      [((0.25, 0.75, 0.5), down, inf, k) for k in (none, 1, 3)] +
                      [((0.75, 0.25, 2.0), down, inf, k) for k in (none, 4)])
    # maxdist: 0, negative, NaN, inf, and one ulp either side of t = 0.5
    t = F(0.5)
    s["maxdist"] = _rays([((0.75, 0.25, 0.5), down, mm, none) for mm in
                          (0.0, -0.0, -1.0, nan, inf, -inf, np.nextafter(t, F(0)), t, np.nextafter(t, one), 1e-45, 3e38)])
    # flat triangles: the box of 0 .. 3 is the slab z = 0, of 6 the slab x = 2; the confinement puts t on the slab's plane
    s["flat"] = _rays([((0.3, 0.2, 0.7), (0.1, 0.05, -1.0), inf, none), ((0.3, 0.2, -0.7), (0.01, 0.02, 0.333), inf, none),
                       ((1.25, 0.3, 0.3), (0.7, 0.01, 0.02), inf, none), ((3.1, 0.3, 0.3), (-0.37, 0.013, 0.021), inf, none),
                       ((0.3, 0.2, 0.7), (0.1, 0.05, -1.0), 0.7, none), ((0.3, 0.2, 1e-3), (0.3, 0.1, -1e-3), inf, none)])
    # zero-area triangles never hit: rays through 7's and 8's points
    s["degenerate"] = _rays([((0.5, 0.25, 0.75), down, 0.4, none), ((0.25, 0.25, 0.75), down, 0.4, none),
                             ((0.5, -1.0, 0.5), (0, 1, 0), 2.0, none), ((0.0, 0.25, 0.5), (1, 0, 0), inf, none)])
    # direction components +0 and -0, and subnormal ones
    z = [0.0, -0.0, 1e-40, -1e-40]
    s["zero_dir"] = _rays([((0.75, 0.25, 0.5), (dx, dy, -1.0), inf, none) for dx in z for dy in z] +
                          [((0.75, 0.25, 0.5), (dx, dy, dz), inf, none) for dx in z[:2] for dy in z[:2] for dz in z[:2]] +
                          [((-1.0, 0.25, 0.0), (1.0, dy, dz), inf, none) for dy in z[:2] for dz in z[:2]])
    # origins on a box plane: x = 0, x = 1, y = 0, z = 0 (on the flat triangles' own plane), z = 1, with zero components
    s["on_box"] = _rays([((0.0, 0.25, 0.5), down, inf, none), ((1.0, 0.25, 0.5), down, inf, none), ((0.5, 0.0, 0.5), down, inf, none),
                         ((0.75, 0.25, 0.0), down, inf, none), ((0.75, 0.25, 0.0), (0, 0, 1), inf, none),
                         ((0.75, 0.25, 1.0), down, inf, none), ((0.75, 0.25, 0.0), (1, 0, 0), inf, none),
                         ((0.0, 0.0, 0.0), (1, 1, 0), inf, none), ((2.0, 0.25, 0.25), (0, 1, 0), inf, none),
                         ((0.0, 0.25, 0.5), (-0.0, 0.0, -1.0), inf, none), ((1.0, 0.25, 0.5), (-0.0, -0.0, -1.0), inf, none)])
    # NaN and inf in origins and directions: no candidate, no hang
    bad = [nan, inf, -inf]
    rows = []
    for b in bad:
        for c in range(3):
            o, d = [0.75, 0.25, 0.5], [0.0, 0.0, -1.0]
            o[c] = b
            rows.append((tuple(o), down, inf, none))
            d[c] = b
            rows.append(((0.75, 0.25, 0.5), tuple(d), inf, none))
            rows.append(((0.75, 0.25, 0.5), tuple(d), 1.0, none))
    rows += [((nan, nan, nan), (nan, nan, nan), nan, none), ((inf, inf, inf), (-inf, -inf, -inf), inf, none),
             ((0.75, 0.25, 0.5), (0.0, 0.0, 0.0), inf, none), ((0.75, 0.25, 0.5), (-0.0, -0.0, -0.0), inf, none),
             ((3e38, 3e38, 3e38), (-1, -1, -1), inf, none), ((0.75, 0.25, 3e38), (0, 0, -3e38), inf, none),
             ((0.75, 0.25, 0.5), (0, 0, -1e-45), inf, none)]
    s["nonfinite"] = _rays(rows)
    return s


def hostile_rays(mesh, seed=11):
    """the streams' kinds of rays against any mesh -> (o, d, m, skip), 64 + rays: axis-parallel rays with signed zeros from points
    of the mesh's vertices' planes, non-finite components, reaches of 0 / NaN / negative"""
    rng = np.random.default_rng(seed)
    V = mesh.V if mesh.nt else np.zeros((1, 3), F)
    rows = []
    zeros, bad = [0.0, -0.0], [np.nan, np.inf, -np.inf]
    for k in range(24):
        p = V[int(rng.integers(0, len(V)))].astype(np.float64)
        axis = k % 3
        o = p + rng.uniform(-0.3, 0.3, 3)
        o[(axis + 1) % 3] = p[(axis + 1) % 3]                        # on a vertex's plane: on box planes of its triangles
        d = [zeros[(k >> 1) & 1], zeros[(k >> 2) & 1], zeros[(k >> 3) & 1]]
        d[axis] = 1.0 if k & 1 else -1.0
        o[axis] -= 2.0 * d[axis]
        rows.append((tuple(o), tuple(d), np.inf, NO_PRIM))
    for k in range(24):
        o, d = list(rng.uniform(-1.5, 1.5, 3)), list(rng.uniform(-1, 1, 3))
        (o if k & 1 else d)[k % 3] = bad[(k // 6) % 3]
        rows.append((tuple(o), tuple(d), np.inf, NO_PRIM))
    for k, mm in enumerate((0.0, -0.0, np.nan, -1.0, np.inf, 1e-30, 0.5, 3.0) * 2):
        o, d = random_rays(rng, 1)
        rows.append((tuple(o[:, 0]), tuple(d[:, 0]), mm, NO_PRIM if k < 8 else int(rng.integers(0, max(mesh.nt, 1)))))
    return _rays(rows)


# ---- rays aimed at a deep tree's stack ---------------------------------------------------------------------------------------------
CORNER_D = (0.3, 0.2, 1.0)


def corner_rays(mesh, bary, d=CORNER_D, tri=0, reverse=False):
    """Rays through points of triangle `tri` (0: the deep grid's corner triangle), barycentrics bary [K, 3], along d [3] or [K, 3],
    from the point minus d (reverse: from the point plus d, along -d) -> o, d [3, K].  Every component of d is positive: the
    point lies in the box of every ancestor of the triangle's leaf, and at every split the ray's near child is the left one,
    which for triangle 0 is the one that holds it -- the ray descends straight to the deepest leaf and holds the sibling of
    every level on the way, depth - 1 entries.  Reversed, the near child is the right one, whose box the ray misses at once
    (it leaves the corner): it is popped before the next push and the ray never holds more than one entry."""
    bary = np.asarray(bary, np.float64).reshape(-1, 3)
    P = np.einsum("kv,vc->kc", bary, mesh.V[mesh.tri[tri].astype(np.int64)].astype(np.float64))
    d = np.broadcast_to(np.asarray(d, np.float64), P.shape)
    o, d = (P + d, -d) if reverse else (P - d, d)
    return np.ascontiguousarray(o.T, F), np.ascontiguousarray(d.T, F)


def cell_prim(i, j, k, n=DEEP_N):
    """the triangle of quad (column i, row j) of an n x n quad_grid: k = 0 under the diagonal (x - x_i >= y - y_j), 1 above it"""
    return 2 * (j * n + i) + k


def deep_stream(mesh):
    """The 577 = 2 * 256 + 64 + 1 rays of the deep tests over deep_grid() -> o, d [3, M], m [M], skip uint32 [M], info: named index
    arrays and, for the vertical rays, the triangle the cell index alone names.
      0            the corner ray, alone in lane 0 of wavefront 0 ..         1 .. 63    .. among random rays
      64 .. 127    a wavefront of corner rays, their points and directions jittered: no two alike
      128 .. 191   a wavefront that alternates corner rays (even lanes) and reversed corner rays
      192 .. 231   two rays from above through each of the 20 extra triangles: a hit at z = 1, the grid below with `last` carried
      232 .. 255   rays along the corner direction through the triangles NEXT to triangle 0 (1 .. 24): they descend towards the
                   corner until a left box misses them and find their hit in a sibling pushed late, at a high stack index
      256 .. 319   vertical rays through barycentric (1/3, 1/3, 1/3) of known cells
      320 .. 383   hostile_rays;  384 .. 576: random rays with finite reaches and, for a third, the triangle under them skipped"""
    rng = np.random.default_rng(91)
    M = 577
    o, d = random_rays(rng, M)
    m, skip = np.full(M, np.inf, F), np.full(M, NO_PRIM, np.uint32)
    third = np.full((1, 3), 1.0 / 3.0)
    info = {}

    def put(name, at, od):
        info[name] = np.asarray(at)
        o[:, at], d[:, at] = od

    put("corner", np.array([0]), corner_rays(mesh, third))
    at = np.arange(64, 128)
    b = rng.dirichlet((1, 1, 1), 64) * 0.7 + 0.1
    dj = np.asarray(CORNER_D) + np.stack([0.001 * np.arange(64), 0.0005 * np.arange(64), 0.002 * np.arange(64)], axis=1)
    put("corner_wave", at, corner_rays(mesh, b, dj))
    b = rng.dirichlet((1, 1, 1), 64) * 0.7 + 0.1
    put("corner_even", np.arange(128, 192, 2), corner_rays(mesh, b[0::2], dj[0::2]))
    put("reversed", np.arange(129, 192, 2), corner_rays(mesh, b[1::2], dj[1::2], reverse=True))
    at = np.arange(192, 232)
    e = (1 << 21) + np.arange(40) // 2
    P = np.einsum("kv,kvc->kc", rng.dirichlet((1, 1, 1), 40) * 0.7 + 0.1, mesh.V[mesh.tri[e].astype(np.int64)].astype(np.float64))
    down = np.stack([rng.uniform(-0.02, 0.02, 40), rng.uniform(-0.02, 0.02, 40), -np.ones(40)], axis=1)
    put("above", at, (np.ascontiguousarray((P - down).T, F), np.ascontiguousarray(down.T, F)))
    info["above_prim"] = e.astype(np.uint32)
    at = np.arange(232, 256)
    near = [corner_rays(mesh, rng.dirichlet((1, 1, 1), 1) * 0.7 + 0.1, tri=t) for t in range(1, 25)]
    put("near_corner", at, (np.concatenate([x[0] for x in near], 1), np.concatenate([x[1] for x in near], 1)))
    at = np.arange(256, 320)
    n = DEEP_N
    ci = np.concatenate([[0, n - 1, 0, n - 1, 1, 800, 801, 805], rng.integers(0, n, 56)])
    cj = np.concatenate([[0, n - 1, n - 1, 0, 0, 795, 796, 800], rng.integers(0, n, 56)])
    ck = np.arange(64) % 2
    want = cell_prim(ci, cj, ck)
    P = mesh.V[mesh.tri[want].astype(np.int64)].astype(np.float64).mean(axis=1)
    P[:, 2] = 0.5                                                    # below the extra triangles
    put("vertical", at, (np.ascontiguousarray(P.T, F), np.tile(np.array([[0.0], [0.0], [-1.0]], F), (1, 64))))
    info["vertical_prim"] = want.astype(np.uint32)
    at = np.arange(320, 384)
    ho, hd, hm, hs = hostile_rays(mesh)
    assert ho.shape[1] == 64
    put("hostile", at, (ho, hd))
    m[at], skip[at] = hm, hs
    at = np.arange(384, M)
    m[at] = rng.uniform(0.3, 3.0, at.size).astype(F)
    m[at[rng.random(at.size) < 0.3]] = np.inf
    with np.errstate(all="ignore"):                                  # the triangle under the ray's crossing of z = 0, by cell
        t0 = -o[2, at].astype(np.float64) / d[2, at]
        fx, fy = ((o[c, at] + t0 * d[c, at] + 1.0) * (n / 2.0) for c in (0, 1))
    inside = (t0 > 0) & (fx > 0) & (fx < n) & (fy > 0) & (fy < n)
    qi, qj = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
    under = cell_prim(qi, qj, ((fy - qj) > (fx - qi)).astype(np.int64))
    pick = inside & (rng.random(at.size) < 0.33)
    skip[at[pick]] = under[pick].astype(np.uint32)
    info["random"] = at
    return np.ascontiguousarray(o), np.ascontiguousarray(d), m, skip, info


def copies_rays(K):
    d = (0.1, 0.05, 1.0)
    inner, mid = np.array((0.3, 0.3, 0.225)), np.array((0.5, 0.5, 0.375))        # inside the triangle; the middle of edge v1 v2
    rows = [(tuple(inner - d), d, np.inf, s) for s in (NO_PRIM, 0, K - 1, 1, K)]
    rows += [(tuple(inner + d), tuple(-np.array(d)), 5.0, NO_PRIM), (tuple(mid - d), d, np.inf, NO_PRIM),
             ((-1.0, 0.0, -0.25), (1.0, 0.0, 0.25), np.inf, NO_PRIM),           # along the edge v0 v1, in the plane: det == 0
             ((0.25, 0.25, 0.5), (0.0, 0.0, -1.0), 0.1, NO_PRIM)]                # every box open, the reach before the hit
    return _rays(rows)


def huge_rays(mesh):
    """hostile_rays and random rays, and rays of huge directions through the subnormal triangles about the origin"""
    rng = np.random.default_rng(19)
    ho, hd, hm, hs = hostile_rays(mesh, seed=23)
    o, d = random_rays(rng, 320)
    k = np.arange(3, mesh.nt, 8)[:32]
    P = mesh.V[mesh.tri[k].astype(np.int64)]                        # [32, 3, 3] subnormal
    o[:, :32] = ((P[:, 0] + P[:, 1]) * F(0.5)).T
    d[:, :32] = 0.0
    d[2, :32] = np.where(np.arange(32) % 2, 1e38, 1.0)
    o[2, :32] = np.where(np.arange(32) % 4 < 2, -1e-39, -1.0)
    m = np.full(320, np.inf, F)
    m[64:128] = rng.uniform(0.3, 3.0, 64)
    return np.concatenate([o, ho], 1), np.concatenate([d, hd], 1), np.concatenate([m, hm]), np.concatenate([np.full(320, NO_PRIM, np.uint32), hs])


# ---- numpy tracers over the statement, in the shape the walks' numpy statements take --------------------------------------------
class np_tracer:
    """nearest hits of a walk's list by nearest_np, `last` carried by queue ray across steps; log: every call's Hits"""

    def __init__(self, mesh, rays):
        self.mesh, self.last, self.log = mesh, np.full(rays, NO_PRIM, np.uint32), []

    def __call__(self, ray, origin, dirs, maxdist):
        j = np.asarray(ray).astype(np.int64)
        h = nearest_np(self.mesh, origin, dirs, maxdist, self.last[j])
        hit = h.hit != 0
        self.last[j[hit]] = h.prim[hit]
        self.log.append((j.copy(), h))
        return h
