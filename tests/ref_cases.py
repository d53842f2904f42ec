"""Input sets shared by the reference-pin tests (tests/test_oracle_vs_reference.py on the CPU,
tests/test_gpu_vs_reference.py on the GPU): the mixed generators, cases.ggx_edge with cases.xi_edge, the testsuite's
ten parameter presets, and named adversarial sets none of the generators produces.  Each builder returns
{name: (closure inputs, xi [2, n])}; the names become the test ids."""
from __future__ import annotations

import numpy as np

import cases

N_MIXED = 1 << 18
N_EDGE = 1 << 16
N_SET = 2048                    # points per preset / adversarial set

ONE_M = np.nextafter(np.float32(1.0), np.float32(0.0))          # 1 - 2^-24
EPS = np.float32(1e-4)                                           # AI_EPSILON
f32 = np.float32


def exiting(wo, N):
    """the reference's switch (src/rlGgx.h:137) in the same fp32 operations: !(dot(N, Rd) < AI_EPSILON), Rd = -wo"""
    Rd = (-wo).astype(np.float32)
    d = (N[0] * Rd[0] + N[1] * Rd[1]) + N[2] * Rd[2]
    return (~(d < EPS)).astype(np.uint8)


def _axis_frames(n):
    """axis-aligned frames (N, T), cycling over +-x, +-y, +-z: dot(N, v) is then one component of v exactly"""
    E = np.eye(3, dtype=np.float32)
    Ns = [E[2], -E[2], E[0], -E[0], E[1], -E[1]]
    Ts = [E[0], E[1], E[1], E[2], E[2], E[0]]
    k = np.arange(n) % 6
    N = np.stack([Ns[i] for i in k], axis=1).astype(np.float32)
    T = np.stack([Ts[i] for i in k], axis=1).astype(np.float32)
    return N, T


def _wo_at(N, T, t, phi):
    """unit-ish wo with dot(N, -wo) == t exactly on an axis frame: wo = s cos(phi) T + s sin(phi) (N x T) - t N"""
    B = np.cross(N.T, T.T).T.astype(np.float32)
    s = np.sqrt(np.float32(1) - t * t).astype(np.float32)
    wo = (s * np.cos(phi).astype(np.float32)) * T + (s * np.sin(phi).astype(np.float32)) * B
    return np.where(N != 0, -t * N, wo).astype(np.float32)


def _base(n, seed=cases.SEED_EDGE):
    wo, N, T = cases.frame(seed, n)
    x = cases.xi(seed, n, 2)
    return dict(wo=wo, N=N, T=T), x


def _ggx_adversarial():
    """named sets (GGX closure inputs, xi): each is the mixed generator with one input pinned to an edge"""
    n = N_SET
    out = {}
    d0 = cases.ggx_mixed(cases.SEED_EDGE, n)
    x0 = cases.xi(cases.SEED_EDGE, n, 2)

    def put(name, xi=None, **over):
        d = dict(d0)
        d.update({k: (np.full(n, v, np.float32) if np.ndim(v) == 0 else v) for k, v in over.items()})
        out[name] = (d, x0 if xi is None else xi)

    for lbl, v in (("0", f32(0)), ("2^-24", f32(2.0 ** -24)), ("0.5", f32(0.5)), ("1-2^-24", ONE_M)):
        put(f"xi0={lbl}", xi=np.stack([np.full(n, v, np.float32), x0[1]]))
        put(f"xi1={lbl}", xi=np.stack([x0[0], np.full(n, v, np.float32)]))
    # roughness floors: alpha = max(1e-4, r^2 ...) -> r = 0.01; mRoughness = max(1e-5, r^2) -> r ~ 0.00316
    for lbl, v in (("0", f32(0)), ("below_alpha_floor", f32(0.005)), ("at_alpha_floor", f32(0.01)),
                   ("above_alpha_floor", np.nextafter(f32(0.01), f32(1))), ("at_G1_floor", f32(np.sqrt(1e-5))),
                   ("1", f32(1))):
        put(f"roughness={lbl}", roughness=v)
    for v in (0.0, 0.5, 0.999, 1.0):
        put(f"anisotropic={v}", anisotropic=f32(v))
    for lbl, v in (("1", f32(1)), ("1+ulp", np.nextafter(f32(1), f32(2))), ("1-ulp", np.nextafter(f32(1), f32(0))),
                   ("1e-5_floored", f32(1e-5)), ("0.6_tir", f32(0.6))):
        put(f"ior={lbl}", ior=v)
    # the entering / exiting switch: dot(N, Rd) at 0, +-AI_EPSILON and one ulp either side of +AI_EPSILON
    N, T = _axis_frames(n)
    phi = (cases.xi(3, n, 1)[0] * f32(6.2831853)).astype(np.float32)
    for lbl, t in (("0", f32(0)), ("+eps", EPS), ("-eps", -EPS), ("eps-ulp", np.nextafter(EPS, f32(0))),
                   ("eps+ulp", np.nextafter(EPS, f32(1)))):
        put(f"dot(N,Rd)={lbl}", wo=_wo_at(N, T, t, phi), N=N, T=T)
    put("wo==N", wo=d0["N"].copy())
    return out


def indir_sets(wo, N, n):
    """eval / pdf directions none of the samplers produce: zero, below the horizon, equal to wo"""
    below = (-(wo * N).sum(axis=0) * N + (wo - (wo * N).sum(axis=0) * N) - f32(0.3) * N).astype(np.float32)
    return {"indir=0": np.zeros((3, n), np.float32), "indir_below": below, "indir=wo": wo.copy()}


def ggx_sets(n_mixed=N_MIXED):
    sets = {"mixed": (cases.ggx_mixed(cases.SEED_PARITY, n_mixed), cases.xi(cases.SEED_PARITY, n_mixed, 2)),
            "edge": (cases.ggx_edge(cases.SEED_EDGE, N_EDGE), cases.xi_edge(cases.SEED_EDGE, N_EDGE))}
    for name, p in cases.GGX_PRESETS.items():
        b, x = _base(N_SET)
        sets[f"preset_{name}"] = (dict(b, **p), x)
    sets.update(_ggx_adversarial())
    return sets


def disney_sets(n_mixed=N_MIXED):
    sets = {"mixed": (cases.disney_mixed(cases.SEED_PARITY, n_mixed), cases.xi(cases.SEED_PARITY, n_mixed, 2))}
    e = cases.ggx_edge(cases.SEED_EDGE, N_EDGE)
    de = cases.disney_mixed(cases.SEED_EDGE, N_EDGE)
    de.update(wo=e["wo"], roughness=e["roughness"])
    sets["edge"] = (de, cases.xi_edge(cases.SEED_EDGE, N_EDGE))
    for name, p in cases.DISNEY_PRESETS.items():
        b, x = _base(N_SET)
        sets[f"preset_{name}"] = (dict(b, **p), x)
    n = N_SET
    d0 = cases.disney_mixed(cases.SEED_EDGE, n)
    x0 = cases.xi(cases.SEED_EDGE, n, 2)

    def put(name, xi=None, **over):
        d = dict(d0)
        d.update({k: (np.full(n, v, np.float32) if np.ndim(v) == 0 else v) for k, v in over.items()})
        sets[name] = (d, x0 if xi is None else xi)

    for lbl, v in (("0", f32(0)), ("2^-24", f32(2.0 ** -24)), ("0.5", f32(0.5)), ("1-2^-24", ONE_M)):
        put(f"xi0={lbl}", xi=np.stack([np.full(n, v, np.float32), x0[1]]))
        put(f"xi1={lbl}", xi=np.stack([x0[0], np.full(n, v, np.float32)]))
    # alpha floor 1e-2 -> roughness 0.1; roughness 1 takes GTR1's a2 == 1 branch (src/rlDisney.cpp:397)
    for lbl, v in (("0", f32(0)), ("below_alpha_floor", f32(0.05)), ("at_alpha_floor", f32(0.1)),
                   ("above_alpha_floor", np.nextafter(f32(0.1), f32(1))), ("1", f32(1))):
        put(f"roughness={lbl}", roughness=v)
    for v in (0.0, 0.5, 0.999, 1.0):
        put(f"anisotropic={v}", anisotropic=f32(v))
    put("clearcoat=1", clearcoat=f32(1))
    put("clearcoat=0", clearcoat=f32(0))
    put("metallic=1", metallic=f32(1))
    put("base_color=0", base_color=np.zeros((3, n), np.float32))
    N, T = _axis_frames(n)
    phi = (cases.xi(3, n, 1)[0] * f32(6.2831853)).astype(np.float32)
    for lbl, t in (("0", f32(0)), ("+eps", EPS), ("-eps", -EPS), ("eps-ulp", np.nextafter(EPS, f32(0))),
                   ("eps+ulp", np.nextafter(EPS, f32(1)))):
        put(f"dot(N,Rd)={lbl}", wo=_wo_at(N, T, t, phi), N=N, T=T)
    put("wo==N", wo=d0["N"].copy())
    return sets


def sss_sets(n_mixed=N_MIXED):
    sets = {}
    m = cases.sss_mixed(cases.SEED_PARITY, n_mixed)
    sets["mixed"] = (dict(dist=m["dist"], albedo=m["albedo"], N=m["N"], T=m["T"]), cases.xi(cases.SEED_PARITY, n_mixed, 2))
    e = cases.sss_mixed(cases.SEED_EDGE, N_EDGE)
    sets["edge"] = (dict(dist=e["dist"], albedo=e["albedo"], N=e["N"], T=e["T"]), cases.xi_edge(cases.SEED_EDGE, N_EDGE))
    for name, p in cases.SKIN_PRESETS.items():
        b, x = _base(N_SET)
        sets[f"preset_{name}"] = (dict(dist=p["sss_scatter_dist"], albedo=p["sss_color"], N=b["N"], T=b["T"],
                                       mult=p["sss_dist_multiplier"]), x)
    n = N_SET
    s0 = cases.sss_mixed(cases.SEED_EDGE, n)
    x0 = cases.xi(cases.SEED_EDGE, n, 2)
    base = dict(dist=s0["dist"], albedo=s0["albedo"], N=s0["N"], T=s0["T"])

    def put(name, xi=None, **over):
        sets[name] = (dict(base, **over), x0 if xi is None else xi)

    for lbl, v in (("0", f32(0)), ("2^-24", f32(2.0 ** -24)), ("0.5", f32(0.5)), ("1-2^-24", ONE_M),
                   ("0.3333", f32(0.3333)), ("0.6666", f32(0.6666)), ("0.75", f32(0.75))):
        put(f"xi0={lbl}", xi=np.stack([np.full(n, v, np.float32), x0[1]]))
    zero_ch = s0["dist"].copy()
    zero_ch[np.arange(n) % 3, np.arange(n)] = 0
    put("dist_zero_channel", dist=zero_ch)
    put("dist_all_zero", dist=np.zeros((3, n), np.float32))
    put("dist_equal_channels", dist=np.repeat(s0["dist"][:1], 3, axis=0))
    put("dist_below_eps", dist=np.full((3, n), 5e-5, np.float32))
    put("albedo=0", albedo=np.zeros((3, n), np.float32))
    put("albedo=1", albedo=np.ones((3, n), np.float32))
    put("dPdu=0", T=np.zeros((3, n), np.float32))
    return sets
