"""helpers of the shadow rays' hits tests (test_trace_opacity_abi.py, test_gpu_trace_opacity*.py): the numpy float32
restatement of the three nodes' sg->out_opacity and of the fold of the opacities along a shadow ray
(include/rlshaders_amd_trace.h, "Shadow rays' hits"), and the inputs.  Restatement only: the reference's shader_evaluate cannot
be run against the stand-in, whose AiShaderGlobalsApplyOpacity aborts."""
import numpy as np

F = np.float32
SHADOW = 0x02                                                 # RLS_RT_SHADOW
# the ray types the bounce tests mix: camera, diffuse, glossy, refracted, shadow, shadow | glossy, every bit
RAY_TYPES = np.array([0x01, 0x20, 0x40, 0x08, 0x02, 0x42, 0xFF], np.uint8)
DENORMAL = np.frombuffer(np.uint32(1).tobytes(), F)[0]
HOSTILE = np.array([0.0, -0.0, -0.25, -3.0, 1.0, 1.5, 7.0, np.nan, np.inf, -np.inf, DENORMAL, -DENORMAL, 1e-30, 3e38, 0.5], F)


def clamp(v):
    """the stand-in's MAX(0, MIN(v, 1)) over a < b ? a : b and a > b ? a : b: a NaN gives 1, -0 stays -0"""
    with np.errstate(invalid="ignore"):
        m = np.where(v < F(1), v, F(1)).astype(F)
        return np.where(F(0) > m, F(0), m).astype(F)


def shadow_mask(ray_type, n):
    return np.zeros(n, bool) if ray_type is None else (ray_type[:n] & SHADOW) != 0


def _col(p, ids, count, n):
    """a parameter at every point: a number, a tuple, a per-point plane, or a per-material column behind ids"""
    if not isinstance(p, np.ndarray):
        return np.repeat(np.asarray(p, F)[..., None], n, axis=-1)
    return p if ids is None else p[..., np.minimum(ids.astype(np.int64) & 0xFFFFFFFF, count - 1)]


def ggx_opacity(n, opacity, opacity_color, KtColor, Kt, ray_type=None, ids=None, count=0):
    with np.errstate(invalid="ignore", over="ignore"):
        o = (_col(opacity, ids, count, n)[None, :] * _col(opacity_color, ids, count, n)).astype(F)
        t = (_col(KtColor, ids, count, n) * _col(Kt, ids, count, n)[None, :]).astype(F)
        return np.where(shadow_mask(ray_type, n)[None, :], (F(1) - t).astype(F), clamp(o)).astype(F)


def disney_opacity(n, opacity, ray_type=None, ids=None, count=0):
    o = _col(opacity, ids, count, n).astype(F)
    return np.where(shadow_mask(ray_type, n)[None, :], o, clamp(o)).astype(F)


def skin_opacity(n, opacity, opacity_color, ray_type=None, incoming=None, ids=None, count=0):
    with np.errstate(invalid="ignore", over="ignore"):
        c = clamp((_col(opacity, ids, count, n)[None, :] * _col(opacity_color, ids, count, n)).astype(F))
        if incoming is None:
            return c
        return np.where(shadow_mask(ray_type, n)[None, :], (incoming[:, :n] * c).astype(F), c).astype(F)


def fold(rays, count, opacity, max_hits, stride, index=None, base=None):
    """T = base or 1; for k < min(count, max_hits): T = T * (1 - o(k * stride + j)); a loop over k, vectorised over the rays.
    opacity: [3, max_hits * stride] per element, or with index [max_hits * stride] a table [3, table_count]"""
    T = np.ones((3, rays), F) if base is None else base[:, :rays].astype(F).copy()
    cnt = np.minimum(count[:rays].astype(np.int64), max_hits)
    j = np.arange(rays)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(cnt.max()) if rays else 0):
            m = cnt > k
            e = k * stride + j[m]
            if index is not None:
                e = np.minimum(index[e].astype(np.int64) & 0xFFFFFFFF, opacity.shape[1] - 1)
            T[:, m] = (T[:, m] * (F(1) - opacity[:, e]).astype(F)).astype(F)
    return T


def same_bits(a, b, nan_bits=False):
    """the same float32 words: every sign of zero, infinity and denormal included.  A NaN must stand where a NaN stands; its
    sign and payload are compared only with nan_bits (two results of the device).  IEEE 754 leaves the NaN an invalid operation
    (inf * 0, inf - inf) delivers to the implementation -- the host's has the sign bit set, the device's has not -- so the numpy
    restatement is no reference for those bits.  What differs is printed (pytest shows it with the failure)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        print("shapes", a.shape, b.shape)
        return False
    d = a.view(np.uint32) != b.view(np.uint32)
    if not nan_bits:
        d &= ~(np.isnan(a) & np.isnan(b))
    if d.any():
        at = np.argwhere(d)[:6]
        print("words differing:", int(d.sum()), "of", d.size, "first at", at.tolist(),
              [(hex(a.view(np.uint32)[tuple(i)]), hex(b.view(np.uint32)[tuple(i)])) for i in at])
    return not d.any()


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def values(seed, *shape, hostile=False):
    """float32 in (-0.25, 1.25) -- both clamp edges are crossed; hostile: every seventh word one of HOSTILE"""
    rng = np.random.default_rng(seed)
    v = (rng.random(shape, F) * F(1.5) - F(0.25)).astype(F)
    if hostile:
        flat = v.reshape(-1)
        at = np.arange(0, flat.size, 7)
        flat[at] = HOSTILE[(at // 7) % HOSTILE.size]
    return v


def ray_types(seed, n, kind):
    """None; every point a shadow ray's; the bounce tests' mix"""
    if kind == "none":
        return None
    if kind == "shadow":
        return np.full(n, SHADOW, np.uint8)
    return RAY_TYPES[np.random.default_rng(seed).integers(0, RAY_TYPES.size, n)]


def counts(seed, rays, max_hits):
    """0, 1, max_hits, max_hits + 1 and 255 among uniform counts 0 .. max_hits; the first and last ray take an extreme"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, max_hits + 1, rays).astype(np.uint8)
    special = np.array([0, 1, max_hits, min(max_hits + 1, 255), 255], np.uint8)
    at = np.arange(0, rays, 5)
    c[at] = special[(at // 5) % special.size]
    if rays:
        c[-1] = 255
    return c
