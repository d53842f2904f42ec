"""Inputs of the tests of the workgroup-shared uniform-slope pass (rlshaders_amd/csrc_rr/: ggx_rr_wg_kernel, what
rls_ggx_reflect_refract launches for a streamed closure in EXACT mode when librls_ggx_rr.so lies beside the product library),
and the frozen arm they are compared with.

A case is (closure dict, xi [4, n]); `case(name)` builds it from its name alone, so the process that runs the frozen kernel
(RLS_GGX_RR_WG=0 is read once per process: `python tests/rr_wg_util.py OUTDIR` is that process) and the test process build
the same inputs.  A "request" is a sample that takes the reference's uniform fallback (src/rlGgx.cpp:27, 38): the stretched
view within 1e-4 of the normal, or |A^2 - 1| < 1e-4.  `requests()` restates the two tests in float64 from twin64.Ggx64.

Recipes (one 256-point workgroup tile, "@tile", or the same 256-point pattern at offset 192 of 512 points, "@straddle": its
first wavefront is the last of tile 0, the rest the first three of tile 1):
  near-normal point: wo = N, roughness 0.1 -- both of its samples are requests;
  quiet point: wo = normalize(N + T), roughness 0.5, isotropic, rx and rx2 in [0.3, 0.6) -- no request (G1 = 0.985 there;
  A = 2 rx / G1 - 1 stays inside (-0.4, 0.22))."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

import cases
import twin64

F = np.float32
ROOT = Path(__file__).resolve().parent.parent
SEED = cases.SEED_PARITY
TILE = 256
NAMES = ("wi", "f", "pdf", "fresnel", "wt", "weight")

SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 513, 8 * 256 + 1, (1 << 16) + 77)
# near-normal points of the 256-point pattern, by recipe
RECIPES = {
    "none": [],
    "one": [100],
    "n32": list(range(3, 256, 8)),                      # 32 points = 64 requests: exactly one pass
    "n33": list(range(3, 256, 8)) + [4],                # 33 points = 66 requests: the first case over one pass
    "all": list(range(256)),                            # 512 requests: eight passes, the queue full
    "first_wave": list(range(0, 64)),                   # every request in one wavefront
    "last_wave": list(range(192, 256)),                 # requests in the last wavefront only
}
LAYOUTS = {"tile": (256, 0), "straddle": (512, 192)}
ROUNDS_N = (1 << 21) + (1 << 19) + 77                 # two and a half rounds of a grid capped at one workgroup per CU x 16


def mixed(n, first=0):
    return cases.ggx_mixed(SEED, n, first), cases.xi(SEED, n, 4, first)


def _quiet(c, x, m):
    """make the points of mask m quiet (see the module docstring)"""
    v = c["N"] + c["T"]
    v = (v / np.linalg.norm(v, axis=0, keepdims=True)).astype(F)
    c["wo"] = np.where(m, v, c["wo"]).astype(F)
    c["roughness"] = np.where(m, F(0.5), c["roughness"]).astype(F)
    c["anisotropic"] = np.where(m, F(0.0), c["anisotropic"]).astype(F)
    for k in (0, 2):
        x[k] = np.where(m, (F(0.3) + F(0.3) * x[k]).astype(F), x[k])


def _near_normal(c, m):
    c["wo"] = np.where(m, c["N"], c["wo"]).astype(F)
    c["roughness"] = np.where(m, F(0.1), c["roughness"]).astype(F)


def recipe(name, layout):
    n, off = LAYOUTS[layout]
    c, x = mixed(n)
    _quiet(c, x, np.ones(n, bool))
    m = np.zeros(n, bool)
    m[off + np.array(RECIPES[name], int)] = True
    _near_normal(c, m)
    return c, x


def rx_zero(sample):
    """the other trigger: rx = 0 makes A = -1.  On the reflect sample only (sample 0) or the refract sample only (1) of every
    third point of two quiet tiles and a partial one, so n1 != n2 in those lanes"""
    n = 2 * TILE + 37
    c, x = mixed(n)
    _quiet(c, x, np.ones(n, bool))
    x[2 * sample][::3] = F(0.0)
    return c, x


def hostile(poison=True):
    """NaN, +-inf, values outside [0, 1) and the other specials of tests/test_gpu_hostile_inputs.py in 4 % of the words of the
    four xi planes and of roughness, over a mix of requesting and quiet lanes (poison=False: the clean run)"""
    from test_gpu_hostile_inputs import SPECIAL
    n = 9 * TILE + 101
    c, x = mixed(n)
    k = np.arange(n)
    _quiet(c, x, (k // 32) % 3 == 0)
    _near_normal(c, k % 5 == 0)
    touched = np.zeros(n, bool)
    if poison:
        rng = np.random.default_rng(23)
        for a in (x[0], x[1], x[2], x[3], c["roughness"]):
            j = rng.choice(n, n // 25, replace=False)
            a[j] = SPECIAL[rng.integers(0, SPECIAL.size, j.size)]
            touched[j] = True
    return c, x, touched


def rounds():
    """a batch a capped grid walks in two and a half rounds, with whole tiles that hold no request between the mixed ones:
    the LDS queue and the two count buffers are reused tile after tile, on both sides of the total == 0 branch"""
    c, x = mixed(ROUNDS_N, first=1 << 33)
    tile = np.arange(ROUNDS_N) // TILE
    _quiet(c, x, (tile % 3 == 1) | (tile % 8 == 6))
    return c, x


def case(name):
    kind, _, arg = name.partition(":")
    if kind == "mixed":
        return mixed(int(arg))
    if kind == "recipe":
        return recipe(*arg.split("@"))
    if kind == "rx0":
        return rx_zero(int(arg))
    if kind == "hostile":
        return hostile(arg == "poisoned")[:2]
    if kind == "rounds":
        return rounds()
    raise KeyError(name)


FROZEN_CASES = ([f"mixed:{n}" for n in SIZES] + [f"recipe:{r}@{l}" for r in RECIPES for l in LAYOUTS] +
                ["rx0:0", "rx0:1", "hostile:poisoned", "rounds:"])


def _view(c):
    """the stretched view of twin64.Ggx64.microfacet (src/rlGgx.cpp:63-80) in float64 -> (g, z', flat, G1, phi)"""
    g = twin64.Ggx64(c)
    cosv = np.clip((g.N * g.wo).sum(0), -1.0, 1.0)
    phiv = np.arctan2((g.V * g.wo).sum(0), (g.U * g.wo).sum(0))
    sinv = np.sqrt(np.maximum(0.0, 1.0 - cosv * cosv))
    l = twin64._norm(np.stack([sinv * np.cos(phiv) * g.ax, sinv * np.sin(phiv) * g.ay, cosv]))
    flat = ~(l[2] < 1.0 - twin64.EPS)
    B = np.tan(np.where(flat, 0.0, np.arccos(np.clip(l[2], -1, 1))))
    return g, l[2], flat, 2.0 / (1.0 + np.sqrt(1.0 + B * B)), np.where(flat, 0.0, np.arctan2(l[1], l[0]))


def requests(c, x):
    """-> (n1, n2): which reflect / refract samples take the uniform fallback; float64 with the threshold comparisons against
    float32(1e-4) -- a recipe keeps every sample a factor of two away from them (margin())"""
    _, _, flat, G1, _ = _view(c)
    out = []
    for rx in (x[0], x[2]):
        A = 2.0 * rx.astype(np.float64) / G1 - 1.0
        out.append(flat | (np.abs(A * A - 1.0) < twin64.EPS))
    return out[0], out[1], flat, G1


def margin(c, x):
    """how far the quantities that decide a request are from their thresholds, as a factor (>= 2: the float64 decision above is
    the float32 one): 1 - z' against 1e-4 and |A^2 - 1| against 1e-4, over all points and both samples"""
    _, z, flat, G1, _ = _view(c)
    ratio = lambda d: np.maximum(d / twin64.EPS, twin64.EPS / np.maximum(d, 1e-300))
    with np.errstate(all="ignore"):
        f = ratio(1.0 - z)
        for rx in (x[0], x[2]):
            A = 2.0 * rx.astype(np.float64) / G1 - 1.0
            f = np.minimum(f, np.where(flat, np.inf, ratio(np.abs(A * A - 1.0))))
    return float(f.min())


def uniform_microfacet(c, rx, ry):
    """the microfacet normal the uniform fallback gives (src/rlGgx.cpp:18-25, 89-98), float64, whether or not the point takes it"""
    g, _, _, _, phi = _view(c)
    rx, ry = rx.astype(np.float64), ry.astype(np.float64)
    r = np.sqrt(rx / (1.0 - rx))
    sx, sy = r * np.cos(2 * np.pi * ry), r * np.sin(2 * np.pi * ry)
    co, si = np.cos(phi), np.sin(phi)
    ox, oy = -(co * sx - si * sy) * g.ax, -(si * sx + co * sy) * g.ay
    return twin64._norm(ox * g.U + oy * g.V + g.N)


def per_tile_requests(c, x):
    n1, n2, _, _ = requests(c, x)
    r = n1.astype(int) + n2.astype(int)
    pad = (-r.size) % TILE
    return np.concatenate([r, np.zeros(pad, int)]).reshape(-1, TILE).sum(1)


# ---- the two arms ----------------------------------------------------------------------------------------------------------------
def run(ctx, c, x, out=None):
    """rls_ggx_reflect_refract on a streamed closure -> the twelve output planes as six host arrays"""
    from gpu_util import dev, ggx_sampler, host
    s = ggx_sampler(ctx, c)
    return [host(t) for t in s.reflectRefract(*(dev(x[k]) for k in range(4)), out=out)]


def companion_loaded():
    """librls_ggx_rr.so is mapped into this process: the product library found it and hands it the streamed EXACT launches"""
    return "librls_ggx_rr.so" in Path("/proc/self/maps").read_text()


def differing_words(a, b):
    """words that differ between two results, NaN equal to NaN by bit pattern, no point excluded"""
    return sum(int((np.ascontiguousarray(p).view(np.uint32) != np.ascontiguousarray(q).view(np.uint32)).sum())
               for p, q in zip(a, b))


def frozen_results(outdir):
    """run every case of FROZEN_CASES through the frozen kernel in a process of its own -> {name: [six arrays]} (lazily read)"""
    env = dict(os.environ, RLS_GGX_RR_WG="0")
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(outdir)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])

    class Lazy(dict):
        def __missing__(self, name):
            with np.load(Path(outdir) / (name.replace(":", "_").replace("@", "_") + ".npz")) as z:
                self[name] = [z[k] for k in NAMES]
            return self[name]
    return Lazy()


def _main(outdir):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import rlshaders_amd as R
    assert os.environ.get("RLS_GGX_RR_WG") == "0"
    R.load()
    ctx = R.Context(0)
    for name in FROZEN_CASES:
        c, x = case(name)
        got = run(ctx, c, x)
        np.savez(Path(outdir) / (name.replace(":", "_").replace("@", "_") + ".npz"), **dict(zip(NAMES, got)))
    ctx.close()
    assert not companion_loaded(), "RLS_GGX_RR_WG=0 must keep the companion out of the process"


if __name__ == "__main__":
    _main(sys.argv[1])
