"""helpers of the instanced-scene library's tests (test_nearest_group_*.py, test_gpu_nearest_group*.py): group_np, the float32
numpy statement of rls_nearest_group_hits (include/rlshaders_amd_nearest_group.h) -- every triangle of every instance that takes
part against every ray, no tree --, a float64 brute force to hold it to, the matrix maps and the world box, instance sets
(exact transforms, general ones, a line of one-triangle instances) and baking a group into one flat mesh.  The meshes and the
hostile ray streams are nearest_util's.  pytest does not collect this module."""
import numpy as np

import nearest_util as U
from nearest_util import F, NO_PRIM

NO_INSTANCE = 0xFFFFFFFF
MAX_INSTANCES = 1 << 16
GROUP_STACK = 16
PAD = F(2.0 ** -21)
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F)


# ---- the maps: a matrix is float32 [3, 4]; p a list of three float32 arrays (or scalars) -----------------------------------------------
def mat_vector(M, p):
    return [(M[c, 0] * p[0] + M[c, 1] * p[1]) + M[c, 2] * p[2] for c in range(3)]


def mat_point(M, p):
    return [((M[c, 0] * p[0] + M[c, 1] * p[1]) + M[c, 2] * p[2]) + M[c, 3] for c in range(3)]


def mat_normal(M, n):
    return [(M[0, c] * n[0] + M[1, c] * n[1]) + M[2, c] * n[2] for c in range(3)]


def mesh_box(mesh):
    """the union of the triangles' boxes -> lo, hi float32 [3] (by value the scene's root box); None for no triangles"""
    if mesh.nt == 0:
        return None
    P = mesh.V[mesh.tri.astype(np.int64).reshape(-1)]
    return P.min(axis=0).astype(F), P.max(axis=0).astype(F)


def world_box(B, lo, hi):
    """W of the mesh box [lo, hi] under B: the eight corners as points, folded from corner 0 to 7, each end widened by e_c 2^-21.
    B: float32 [3, 4] -> wlo, whi [3]; or [n, 3, 4], many placements of one box at once -> [n, 3] each"""
    B = np.asarray(B, F)
    Bt = np.moveaxis(B, (-2, -1), (0, 1))                              # [3, 4, ...]: Bt[c, k] a scalar or an array over placements
    with np.errstate(all="ignore"):
        wlo = whi = None
        for k in range(8):
            p = [hi[c] if k & (1 << c) else lo[c] for c in range(3)]
            q = mat_point(Bt, p)
            wlo = q if k == 0 else [U._min(wlo[c], q[c]) for c in range(3)]
            whi = q if k == 0 else [U._max(whi[c], q[c]) for c in range(3)]
        m = [U._max(np.abs(lo[c]), np.abs(hi[c])) for c in range(3)]
        out_lo, out_hi = [], []
        for c in range(3):
            e = ((np.abs(Bt[c, 0]) * m[0] + np.abs(Bt[c, 1]) * m[1]) + np.abs(Bt[c, 2]) * m[2]) + np.abs(Bt[c, 3])
            pad = (e * PAD).astype(F)
            out_lo.append(np.asarray(wlo[c], F) - pad)
            out_hi.append(np.asarray(whi[c], F) + pad)
    return np.stack(out_lo, axis=-1).astype(F), np.stack(out_hi, axis=-1).astype(F)


class Inst:
    """an instance: mesh (a nearest_util.Mesh), B = to_world, A = to_object float32 [3, 4] (None: the float64 inverse of B
    rounded), surface_base; W and parked follow from them"""

    def __init__(self, mesh, B=IDENTITY, A=None, base=0, world=None):
        """world: (wlo, whi) where the caller has them (world_box over many placements at once)"""
        self.mesh, self.base = mesh, int(base)
        B64 = np.asarray(B, np.float64).reshape(3, 4)
        with np.errstate(all="ignore"):
            if A is None:
                A = np.linalg.inv(np.vstack([B64, [0, 0, 0, 1]]))[:3]
            self.B, self.A = B64.astype(F), np.asarray(A, np.float64).reshape(3, 4).astype(F)
        box = mesh_box(mesh) if world is None else ()
        self.parked = box is None or not (np.isfinite(self.A).all() and np.isfinite(self.B).all())
        self.wlo, self.whi = np.zeros(3, F), np.zeros(3, F)
        if not self.parked:
            wlo, whi = world_box(self.B, *box) if world is None else world
            if np.isfinite(wlo).all() and np.isfinite(whi).all():
                self.wlo, self.whi = wlo, whi
            else:
                self.parked = True


# ---- the statement -----------------------------------------------------------------------------------------------------------------
def _interval(lo, hi, o, inv, sign, tn, tf):
    """the box interval from (tn, tf): lo[c], hi[c] broadcast against o[c] [K]"""
    for c in range(3):
        a, b = (lo[c] - o[c]) * inv[c], (hi[c] - o[c]) * inv[c]
        a, b = np.where(sign[c], b, a), np.where(sign[c], a, b)
        tn = np.where(a > tn, a, tn)
        tf = np.where(b < tf, b, tf)
    return tn, tf


def _candidates(v0, v1, v2, o, d, inv, sign, tn0, tf0):
    """nearest_util._candidate with the interval started at (tn0, tf0) [K]; v0[c], v1[c], v2[c]: float32 [nt, 1] -- every triangle
    against every ray, [nt, K], the same float32 operations in the same order elementwise"""
    lo, hi = [U._min(U._min(v0[c], v1[c]), v2[c]) for c in range(3)], [U._max(U._max(v0[c], v1[c]), v2[c]) for c in range(3)]
    tn, tf = _interval(lo, hi, o, inv, sign, tn0, tf0)
    box = ~(tn > tf)
    e1, e2 = [v1[c] - v0[c] for c in range(3)], [v2[c] - v0[c] for c in range(3)]
    p = U._cross(d, e2)
    det = U._dot(e1, p)
    r = F(1) / det
    s = [o[0] - v0[0], o[1] - v0[1], o[2] - v0[2]]
    u = U._dot(s, p) * r
    q = U._cross(s, e1)
    v = U._dot(d, q) * r
    tm = U._dot(e2, q) * r
    tri_hit = ((det < 0) | (det > 0)) & (u >= 0) & (v >= 0) & (u + v <= F(1)) & ~np.isnan(tm)
    t = tm
    t = np.where(tn > t, tn, t)
    t = np.where(tf < t, tf, t)
    return box, tri_hit, t, u, v


def group_np(insts, o, d, m=None, skip=None, chunk=1 << 22):
    """The statement: o, d float32 [3, M]; m float32 [M] or None (+inf); skip: (skip_instance, skip_prim) uint32 [M] each, or
    None.  -> nearest_util.Hits with `instance` uint32 [M] beside prim; surface is the based id.  Instances in ascending j, and
    within one the triangles in ascending i: a tie keeps the smaller j, then the smaller i."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    M = o.shape[1]
    m = np.full(M, np.inf, F) if m is None else np.asarray(m, F)
    if skip is None:
        skip_j, skip_i = np.full(M, NO_INSTANCE, np.int64), np.full(M, NO_PRIM, np.int64)
    else:
        skip_j, skip_i = (np.asarray(s).astype(np.int64) & 0xFFFFFFFF for s in skip)
    best_t, best_u, best_v = np.zeros(M, F), np.zeros(M, F), np.zeros(M, F)
    best_j, best_i = np.full(M, -1, np.int64), np.full(M, -1, np.int64)
    with np.errstate(all="ignore"):
        inv = (F(1) / d).astype(F)
        sign = np.signbit(inv)
        for j, ins in enumerate(insts):
            if ins.parked:
                continue
            tnW, tfW = _interval(ins.wlo, ins.whi, o, inv, sign, np.zeros(M, F), np.full(M, np.inf, F))
            at = np.nonzero(~(tnW > tfW))[0]                          # the rays the instance takes part for
            if at.size == 0:
                continue
            oo = [np.asarray(x, F) for x in mat_point(ins.A, [o[c, at] for c in range(3)])]
            dd = [np.asarray(x, F) for x in mat_vector(ins.A, [d[c, at] for c in range(3)])]
            ii = [(F(1) / dd[c]).astype(F) for c in range(3)]
            ss = [np.signbit(ii[c]) for c in range(3)]
            mesh = ins.mesh
            K = at.size
            bt, bu, bv, bi = np.zeros(K, F), np.zeros(K, F), np.zeros(K, F), np.full(K, -1, np.int64)
            step = max(1, chunk // K)
            for i0 in range(0, mesh.nt, step):
                ix = mesh.tri[i0:i0 + step].astype(np.int64)
                v0, v1, v2 = ([np.ascontiguousarray(mesh.V[ix[:, k], c])[:, None] for c in range(3)] for k in range(3))
                box, tri_hit, t, u, v = _candidates(v0, v1, v2, oo, dd, ii, ss, tnW[at], tfW[at])
                ids = np.arange(i0, i0 + ix.shape[0])[:, None]
                cand = ~((skip_j[at] == j)[None, :] & (skip_i[at][None, :] == ids)) & box & tri_hit & (t > 0) & (t <= m[at][None, :])
                key = np.where(cand, t, np.inf)
                k = np.argmin(key, axis=0)                            # the first of the smallest: the smaller i at a tie
                cols = np.arange(K)
                has = cand.any(axis=0)
                wrong = has & ~cand[k, cols]                          # every candidate at t = +inf and a non-candidate ahead of them
                if wrong.any():
                    k[wrong] = np.argmax(cand[:, wrong], axis=0)
                take = has & ((bi < 0) | (t[k, cols] < bt))
                bt, bu, bv = np.where(take, t[k, cols], bt), np.where(take, u[k, cols], bu), np.where(take, v[k, cols], bv)
                bi = np.where(take, k + i0, bi)
            take = (bi >= 0) & ((best_j[at] < 0) | (bt < best_t[at]))
            sel = at[take]
            best_t[sel], best_u[sel], best_v[sel], best_i[sel], best_j[sel] = bt[take], bu[take], bv[take], bi[take], j
        return _report(insts, o, d, best_j, best_i, best_t, best_u, best_v)


def _report(insts, o, d, best_j, best_i, best_t, best_u, best_v):
    M = o.shape[1]
    hit = best_j >= 0
    h = U.Hits()
    h.hit = hit.astype(np.uint8)
    h.prim, h.instance = np.where(hit, best_i, 0).astype(np.uint32), np.where(hit, best_j, 0).astype(np.uint32)
    h.t, h.u, h.v = best_t.astype(F), best_u.astype(F), best_v.astype(F)
    h.surface = np.zeros(M, np.uint32)
    h.P = np.where(hit, np.stack([o[c] + h.t * d[c] for c in range(3)]), F(0)).astype(F)
    h.wo = np.where(hit, -d, F(0)).astype(F)
    h.N, h.Ns, h.T = np.zeros((3, M), F), np.zeros((3, M), F), np.zeros((3, M), F)
    for j in np.unique(best_j[hit]):
        ins, at = insts[int(j)], np.nonzero(best_j == j)[0]
        mesh = ins.mesh
        prim = best_i[at]
        sid = np.zeros(at.size, np.int64) if mesh.surface is None else mesh.surface[prim].astype(np.int64)
        h.surface[at] = ((sid + ins.base) & 0xFFFFFFFF).astype(np.uint32)
        ix = mesh.tri[prim].astype(np.int64)
        v0, v1, v2 = (mesh.V[ix[:, k]].T for k in range(3))
        e1, e2 = v1 - v0, v2 - v0
        h.N[:, at] = U._normalize([np.asarray(x, F) for x in mat_normal(ins.A, U._cross(e1, e2))])
        h.T[:, at] = U._normalize([np.asarray(x, F) for x in mat_vector(ins.B, e1)])
        if mesh.normals is None:
            h.Ns[:, at] = h.N[:, at]
        else:
            n0, n1, n2 = (mesh.normals[ix[:, k]].T for k in range(3))
            u, v = h.u[at], h.v[at]
            w = (F(1) - u) - v
            s = [(w * n0[c] + u * n1[c]) + v * n2[c] for c in range(3)]
            h.Ns[:, at] = U._normalize([np.asarray(x, F) for x in mat_normal(ins.A, s)])
    return h


def brute64(insts, o, d, m=None):
    """float64 over every instance and triangle, no boxes: the ray mapped by A in float64, nearest_util.brute64 in object space
    (t is shared) -> (hit, instance, prim, t, margin); margin: the smallest of every instance's own margin (an edge, a runner-up,
    a near miss) and the gap in t between the winning instance and the next"""
    o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
    M = o64.shape[1]
    best = np.full(M, np.inf)
    second = np.full(M, np.inf)
    bj, bi = np.zeros(M, np.int64), np.zeros(M, np.int64)
    margin = np.full(M, np.inf)
    for j, ins in enumerate(insts):
        if ins.parked:
            continue
        A = ins.A.astype(np.float64)
        oo, dd = A[:, :3] @ o64 + A[:, 3:4], A[:, :3] @ d64
        hit, k, t, mg = U.brute64(ins.mesh, oo, dd, m)
        t = np.where(hit, t, np.inf)
        margin = np.minimum(margin, mg)
        better = t < best
        second = np.where(better, best, np.minimum(second, t))
        bj, bi, best = np.where(better, j, bj), np.where(better, k, bi), np.where(better, t, best)
    hit = np.isfinite(best)
    margin = np.minimum(margin, np.where(hit, second - best, np.inf))
    return hit, bj, bi, np.where(hit, best, 0.0), margin


# ---- instance sets -------------------------------------------------------------------------------------------------------------------
def affine(L=np.eye(3), t=(0, 0, 0)):
    return np.concatenate([np.asarray(L, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def general_instances(mesh, n, seed=7, spread=None, bases=True, scales=(0.5, 2.0)):
    """n placements of `mesh`: a rotation times a shear times a non-uniform scale (log-uniform in `scales`), centres in a cube of
    half-width `spread` (default: grows with n so that neighbours overlap now and then); surface bases 10 j"""
    rng = np.random.default_rng(seed)
    spread = (1.0 + 0.8 * n ** (1.0 / 3.0)) if spread is None else spread
    out = []
    for j in range(n):
        S = np.diag(np.exp(rng.uniform(np.log(scales[0]), np.log(scales[1]), 3)))
        H = np.eye(3)
        H[0, 1], H[1, 2] = rng.uniform(-0.3, 0.3, 2)
        L = rotation(rng) @ H @ S
        out.append(Inst(mesh, affine(L, rng.uniform(-spread, spread, 3) if n > 1 else (0.1, -0.2, 0.05)), base=10 * j if bases else 0))
    return out


def exact_instances(mesh, n=6, seed=3):
    """placements exact in float32: translations on the grid of 1/4, single-axis mirrors, uniform power-of-two scales -- both
    matrices are exact, and so is every product and sum of a map of dyadic points that stay small"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(n):
        s = float(2.0 ** rng.integers(-1, 2))
        L = np.eye(3) * s
        if j % 3 == 1:
            L[j % 2, j % 2] = -s                                     # a mirror in x or y
        t = rng.integers(-8, 9, 3) / 4.0
        B = affine(L, t)
        A = affine(np.linalg.inv(L), -np.linalg.inv(L) @ t)
        out.append(Inst(mesh, B, A, base=100 * j))
    return out


def line_triangle():
    return U.Mesh([(0, -1, -1), (0, 1, -1), (0, 0, 1)], [(0, 1, 2)], surface=[1])


def line_instances(n, step=1.0):
    """n one-triangle instances along x, the triangle facing -x... +x rays: instance j's triangle in the plane x = j * step"""
    tri = line_triangle()
    if n == 0:
        return []
    B = np.tile(IDENTITY, (n, 1, 1))
    B[:, 0, 3] = np.arange(n) * step
    A = B.copy()
    A[:, 0, 3] = -B[:, 0, 3]
    wlo, whi = world_box(B, *mesh_box(tri))
    return [Inst(tri, B[j], A[j], base=j, world=(wlo[j], whi[j])) for j in range(n)]


def placed(mesh, A, B, bases=None):
    """n placements of ONE mesh at once: A, B float32 [n, 3, 4], the world boxes by world_box over all of them (a NaN or an inf
    among the matrices, or a box that overflows, parks its instance as the statement says); surface bases j unless given"""
    A, B = np.asarray(A, F).reshape(-1, 3, 4), np.asarray(B, F).reshape(-1, 3, 4)
    wlo, whi = world_box(B, *mesh_box(mesh))
    return [Inst(mesh, B[j], A[j], base=j if bases is None else bases[j], world=(wlo[j], whi[j])) for j in range(B.shape[0])]


def coincident():
    """three general placements of the icosphere with instance 0 again as 2 and 5 and instance 1 again as 4, under bases of their
    own: every hit of 0 or 1 ties with its copies at the same t bits, and the smaller j wins"""
    i = general_instances(U.icosphere(1), 3, seed=8)
    return [i[0], i[1], Inst(i[0].mesh, i[0].B, i[0].A, base=50), i[2], Inst(i[1].mesh, i[1].B, i[1].A, base=60),
            Inst(i[0].mesh, i[0].B, i[0].A, base=70)]


# ---- the update's launch plan, read from a top tree's links (rls_nearest_group_update in group.hip) ----------------------------------
BLOCK = 256


def level_sizes(links):
    """links uint32 [top_nodes, 2] (first, meta) of read_tree -> the node count of every level, the root's first"""
    first, count = links[:, 0].astype(np.int64), links[:, 1].astype(np.int64) & 0xFF
    sizes, level = [], np.zeros(1, np.int64)
    while level.size:
        sizes.append(int(level.size))
        inner = first[level[count[level] == 0]]
        level = np.concatenate([inner, inner + 1])
    assert sum(sizes) == links.shape[0]
    return sizes


def update_plan(sizes):
    """-> (wide, folded): the levels from the root down of at most BLOCK nodes each run in ONE single-workgroup launch where there
    are two or more of them (`folded`); every deeper level, and a lone level, is a launch of its own (`wide`)"""
    trailing = 0
    while trailing < len(sizes) and sizes[trailing] <= BLOCK:
        trailing += 1
    folded = trailing if trailing >= 2 else 0
    return len(sizes) - folded, folded


# the update's edge cases (test_gpu_nearest_group_update_edges.py; the plans are pinned on the CPU by test_nearest_group_host.py):
# instances, top leaf -> the node count of every level of the top tree over line_instances(n), the root's first.  Levels of more
# than BLOCK nodes are launched one by one, and so is every level below one; the rest is the single-workgroup launch.
_POWERS = [1, 2, 4, 8, 16, 32, 64, 128, 256]
PLANS = {
    (1, 1): [1],                                                     # depth 1: nothing folded, one level launch
    (2, 1): [1, 2],                                                  # everything folded
    (256, 1): _POWERS,                                               # a deepest level of exactly BLOCK nodes: everything folded
    (257, 1): _POWERS + [2],                                         # one leaf more: a tenth level of two nodes, still all folded
    (384, 1): _POWERS + [256],                                       # two levels of exactly BLOCK nodes: the last all-folded plan
    (385, 1): _POWERS + [258],                                       # the first plan with a wide level (a level grows by two nodes)
    (600, 1): _POWERS + [512, 176],                                  # a wide level of two tiles beside a narrow deepest level
    (1500, 4): _POWERS + [512],                                      # leaves of 2 and 3 records, a wide level of them
    (MAX_INSTANCES, 1): _POWERS + [512 << k for k in range(8)],      # 17 levels, 8 of them wide
}


def line_moves(n, kind):
    """new matrices for line_instances(n), exact in float32 -> A, B float32 [n, 3, 4].  shift: a non-uniform scale and a step of
    3/4; reverse: the line backwards, so that the tree built over the old line holds the instances the wrong way round; point:
    every placement shrunk onto the one point (3, 0, 0) -- every box of the old tree then holds the same box"""
    L, t = np.eye(3), np.zeros((n, 3))
    j = np.arange(n, dtype=np.float64)
    if kind == "shift":
        L = np.diag([1.0, 2.0, 0.5])
        t[:, 0], t[:, 1], t[:, 2] = 0.75 * j + 0.5, 0.25, -0.125
    elif kind == "reverse":
        t[:, 0] = (n - 1) - j
    elif kind == "point":
        L = np.eye(3) * 0.5
        t[:, 0] = 3.0
    else:
        raise ValueError(kind)
    B = np.tile(affine(L), (n, 1, 1))
    B[:, :, 3] = t
    A = np.tile(affine(np.linalg.inv(L)), (n, 1, 1))
    A[:, :, 3] = -t @ np.linalg.inv(L).T
    return A.astype(F), B.astype(F)


def park(A, B, which):
    """in place: the instances `which` (indices) parked three ways in turn -- a NaN in A, an inf in B, and a B of finite entries
    under which the line's triangle (y and z in [-1, 1]) has a world box that overflows"""
    for k, j in enumerate(which):
        r = k // 3
        if k % 3 == 0:
            A[j, r % 3, (r // 3) % 4] = np.nan
        elif k % 3 == 1:
            B[j, r % 3, (r // 3) % 4] = np.inf if r % 2 else -np.inf
        else:
            B[j, 1, 1] = B[j, 1, 2] = F(3e38)
    return A, B


def parked_pattern(n):
    """about one instance in seven, by tile of BLOCK instances: tile 0, 3, 6, .. park none; tile 1, 4, .. every fourth instance
    (16 in each of the tile's four waves); tile 2, 5, .. every other instance of its second wave alone -- and the same goes for
    a last partial tile"""
    j = np.arange(n)
    tile, lane = j // BLOCK, j % BLOCK
    return np.flatnonzero(((tile % 3 == 1) & (lane % 4 == 0)) | ((tile % 3 == 2) & (lane // 64 == 1) & (lane % 2 == 1)))


def line_stream(x_lo, x_hi, K=512, seed=1):
    """K rays along a line of placed triangles between x_lo and x_hi: from points near the axis along +-x with a small drift (they
    cross the next triangle's plane inside it), a tenth of them well off the axis; reaches +inf or about the step
    -> o, d float32 [3, K], m [K]"""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(x_lo - 1.0, x_hi + 1.0, K), rng.uniform(-0.25, 0.45, K), rng.uniform(-0.4, -0.15, K)])
    d = np.stack([rng.choice([-1.0, 1.0], K), rng.uniform(-0.02, 0.02, K), rng.uniform(-0.02, 0.02, K)]) * rng.uniform(0.5, 2.0, K)
    off = rng.random(K) < 0.1
    o[1, off] += 5.0
    m = np.where(rng.random(K) < 0.4, np.inf, rng.uniform(0.2, 3.0, K))
    return o.astype(F), d.astype(F), m.astype(F)


def bake(insts):
    """the group as ONE flat mesh: every vertex mapped by B (float32, the statement's point map), triangle j * nt + i, surface
    based, a vertex normal mapped by A as a normal (where every mesh has them).  Only meaningful where the maps are exact."""
    Vs, Ts, Ss, Ns, off = [], [], [], [], 0
    for ins in insts:
        mesh = ins.mesh
        with np.errstate(all="ignore"):
            Vs.append(np.stack([np.asarray(x, F) for x in mat_point(ins.B, [mesh.V[:, c] for c in range(3)])], axis=1))
            if mesh.normals is not None:
                Ns.append(np.stack([np.asarray(x, F) for x in mat_normal(ins.A, [mesh.normals[:, c] for c in range(3)])], axis=1))
        Ts.append(mesh.tri.astype(np.int64) + off)
        sid = np.zeros(mesh.nt, np.int64) if mesh.surface is None else mesh.surface.astype(np.int64)
        Ss.append((sid + ins.base) & 0xFFFFFFFF)
        off += mesh.V.shape[0]
    return U.Mesh(np.concatenate(Vs), np.concatenate(Ts), surface=np.concatenate(Ss),
                  normals=np.concatenate(Ns) if len(Ns) == len(insts) and insts else None)


def matrices(insts):
    """-> to_object, to_world float32 [n, 12]"""
    return (np.stack([i.A.reshape(12) for i in insts]).astype(F) if insts else np.zeros((0, 12), F),
            np.stack([i.B.reshape(12) for i in insts]).astype(F) if insts else np.zeros((0, 12), F))


# ---- part 3 of test_nearest_group_statement.py: placements across six decades that float32 can still resolve ---------------------
WIDE_SCALES = (1e-3, 2e-3, 1.0, 1.5, 7e2, 1e3)


def wide_instances(mesh, seed, offset=1.0):
    """six placements, a rotation times a shear times a non-uniform scale each, their sizes from 1e-3 to 1e3 in overlapping pairs;
    a placement's centre is as far from the origin as it is large, so that to_object times a world point near it does not cancel"""
    rng = np.random.default_rng(seed)
    out = []
    for j, g in enumerate(WIDE_SCALES):
        S = np.diag(g * np.exp(rng.uniform(np.log(0.5), np.log(2.0), 3)))
        H = np.eye(3)
        H[0, 1], H[1, 2] = rng.uniform(-0.3, 0.3, 2)
        out.append(Inst(mesh, affine(rotation(rng) @ H @ S, g * rng.uniform(-offset, offset, 3)), base=10 * j))
    return out


def cone_rays(rng, mesh, K, dist=2.0, cosmin=0.3):
    """rays at points inside random triangles (barycentrics at least 0.05 from every edge), from `dist` away within the cone of
    cos >= cosmin about the triangle's normal, either side -> o, d float64 [3, K] in the mesh's space (d not normalised)"""
    i = rng.integers(0, mesh.nt, K)
    b = rng.dirichlet((1, 1, 1), K) * (1 - 0.15) + 0.05
    V = mesh.V.astype(np.float64)[mesh.tri[i].astype(np.int64)]
    P = np.einsum("kv,kvc->kc", b, V)
    n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n *= rng.choice([-1.0, 1.0], (K, 1))
    w = rng.normal(size=(K, 3))
    w -= n * np.einsum("kc,kc->k", w, n)[:, None]
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    c = rng.uniform(cosmin, 1.0, (K, 1))
    o = P + dist * (n * c + w * np.sqrt(1 - c * c))
    d = (P - o) * rng.uniform(0.5, 2.0, (K, 1))
    return o.T, d.T


def wide_case(mesh, seed, offset=1.0, K=400):
    """wide_instances and, per instance, K cone_rays mapped to the world by B in float64 -> insts, o, d float32 [3, 6 K]"""
    insts = wide_instances(mesh, seed, offset)
    rng = np.random.default_rng(seed + 100)
    O, D = [], []
    for i in insts:
        o, d = cone_rays(rng, mesh, K)
        B = i.B.astype(np.float64)
        O.append(B[:, :3] @ o + B[:, 3:4])
        D.append(B[:, :3] @ d)
    return insts, np.concatenate(O, 1).astype(F), np.concatenate(D, 1).astype(F)


# ---- ray streams over a group ------------------------------------------------------------------------------------------------------
def group_rays(insts, K, seed, reach=True):
    """K random rays through the group's world box, half of them aimed at points inside triangles of random instances, then the
    hostile rays of the first mesh; reaches about the group's size for most, and NaN / 0 among the hostile ones"""
    rng = np.random.default_rng(seed)
    live = [i for i in insts if not i.parked]
    lo = np.min([i.wlo for i in live], axis=0) if live else -np.ones(3)
    hi = np.max([i.whi for i in live], axis=0) if live else np.ones(3)
    c, r = (lo + hi) / 2, (hi - lo).max() / 2 + 0.5
    o = (c[:, None] + rng.uniform(-1.5 * r, 1.5 * r, (3, K))).astype(F)
    d = ((c[:, None] + rng.uniform(-r, r, (3, K))) - o).astype(F)
    if live:
        t = []
        for k in range(K // 2):
            i = live[int(rng.integers(0, len(live)))]
            p = U.interior_targets(rng, i.mesh, 1, margin=0.0)[0]
            t.append(i.B[:, :3].astype(np.float64) @ p + i.B[:, 3])
        ao, ad = U.rays_at_targets(rng, np.array(t), spread=float(r))
        o[:, :K // 2], d[:, :K // 2] = ao, ad
    m = np.where(rng.random(K) < 0.3, np.inf, rng.uniform(0.3, 3.0, K)).astype(F) if reach else np.full(K, np.inf, F)
    ho, hd, hm, _ = U.hostile_rays(insts[0].mesh if insts else U.single_triangle())
    return np.concatenate([o, ho], 1), np.concatenate([d, hd], 1), np.concatenate([m, hm])


def skips(rng, first):
    """for a third of the rays that hit, the (instance, prim) hit first; for a few, that prim under ANOTHER instance id"""
    n = first.hit.shape[0]
    pick = (first.hit != 0) & (rng.random(n) < 0.4)
    sj = np.where(pick, first.instance, NO_INSTANCE).astype(np.uint32)
    si = np.where(pick, first.prim, NO_PRIM).astype(np.uint32)
    other = pick & (rng.random(n) < 0.25)
    sj[other] += 1
    return sj, si


def line_rays(n):
    """over line_instances(n): ray 0 along the line from x = -1 towards +x (it descends to instance 0 holding
    every level's sibling), ray 1 the same from the far end towards -x, then rays across the line at chosen instances, and rays
    that miss the root -> o, d float32 [3, 8], the instance each hits (NO_INSTANCE: none)"""
    rows = [((-1.0, 0.0, -0.25), (1.0, 0.0, 0.0), 0), ((float(n), 0.0, -0.25), (-1.0, 0.0, 0.0), n - 1)]
    for j in (0, 1, n // 2, n - 1):
        rows.append(((j - 0.5, 0.25, -0.5), (1.0, 0.0, 0.125), j))    # crosses the plane x = j inside its triangle, no other
    rows += [((-1.0, 5.0, 0.0), (1.0, 0.0, 0.0), NO_INSTANCE), ((3.0, 0.0, 4.0), (0.0, 1.0, 0.0), NO_INSTANCE)]
    o = np.array([r[0] for r in rows], F).T
    dd = np.array([r[1] for r in rows], F).T
    return np.ascontiguousarray(o), np.ascontiguousarray(dd), np.array([r[2] for r in rows], np.uint32)
