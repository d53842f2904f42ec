"""helpers shared by the -m gpu tests of the caller-traced integrators (test_gpu_trace_ggx.py, test_gpu_trace_disney.py,
test_gpu_trace_edges.py): the input sets, the queues composed on the CPU per sample (the oracle), the float32 sequential
sum of a resolve."""
import numpy as np
import torch

import cases
import oracle_lib as O

DIFFUSE, GLOSSY = 0x08, 0x10          # RLS_RAY_DIFFUSE, RLS_RAY_GLOSSY
EPS = np.float32(1e-4)                # AI_EPSILON: a sample is valid where pdf > 1e-4 (src/rlDisney.cpp:309)


def exiting(n):
    return (np.arange(n) % 5 == 3).astype(np.uint8)


def ggx_inputs(kind, n):
    """rlGgx: (case dict for the sampler, exiting or None, materials or None)"""
    if kind == "mixed":
        return cases.ggx_mixed(cases.SEED_PARITY, n), None, None
    if kind == "edge":
        return cases.ggx_edge(cases.SEED_EDGE, n), exiting(n), None
    if kind.startswith("preset:"):
        wo, N, T = cases.frame(cases.SEED_PARITY, n)
        return dict(wo=wo, N=N, T=T, **cases.GGX_PRESETS[kind[7:]]), None, None
    if kind == "uniform":
        wo, N, T = cases.frame(cases.SEED_PARITY, n)
        return dict(wo=wo, N=N, T=T, KsColor=(0.9, 0.6, 0.3), roughness=0.4, ior=1.6, anisotropic=0.5), exiting(n), None
    if kind == "materials":
        m = 7
        cols = cases.ggx_mixed(cases.SEED_PARITY + 1, m)
        wo, N, T = cases.frame(cases.SEED_PARITY, n)
        ids = (O.gen_uniform(cases.SEED_PARITY, 0, n, 77) * m).astype(np.uint32) % m
        case = dict(wo=wo, N=N, T=T, KsColor=cols["KsColor"], roughness=cols["roughness"], ior=cols["ior"],
                    anisotropic=cols["anisotropic"])
        return case, None, (torch.from_numpy(ids.astype(np.int32)).cuda(), m)
    raise KeyError(kind)


def disney_inputs(kind, n):
    """rlDisney: (case dict for the sampler, materials or None)"""
    if kind == "mixed":
        return cases.disney_mixed(cases.SEED_PARITY, n), None
    if kind.startswith("preset:"):
        wo, N, T = cases.frame(cases.SEED_PARITY, n)
        return dict(wo=wo, N=N, T=T, **cases.DISNEY_PRESETS[kind[7:]]), None
    if kind == "uniform":
        wo, N, T = cases.frame(cases.SEED_PARITY, n)
        return dict(wo=wo, N=N, T=T, base_color=(0.8, 0.5, 0.3), subsurface=0.1, metallic=0.2, specular=0.5,
                    specular_tint=0.1, roughness=0.35, anisotropic=0.3, sheen=0.2, sheen_tint=0.5, clearcoat=0.3,
                    clearcoat_gloss=0.6), None
    if kind == "materials":
        m = 7
        cols = cases.disney_mixed(cases.SEED_PARITY + 1, m)
        wo, N, T = cases.frame(cases.SEED_PARITY, n)
        ids = (O.gen_uniform(cases.SEED_PARITY, 0, n, 77) * m).astype(np.uint32) % m
        case = dict(cols, wo=wo, N=N, T=T)
        return case, (torch.from_numpy(ids.astype(np.int32)).cuda(), m)
    if kind == "rare":
        # the specular lobe's packed rare branches with every lane asking (test_gpu_disney_config3.py,
        # test_packed_rare_branches_with_every_lane_asking): views along the normal take the uniform-slope fallback,
        # clearcoat = 1 sends samples to the clearcoat half vector
        wo, N, T = cases.frame(cases.SEED_PARITY, n)
        c = cases.disney_mixed(cases.SEED_PARITY, n)
        return dict(c, wo=N.copy(), N=N, T=T, clearcoat=np.ones(n, np.float32)), None
    if kind == "metallic_mix":
        # every third point metallic = 1: no diffuse lobe there, the diffuse counts vary between 0 and spp
        c = cases.disney_mixed(cases.SEED_PARITY, n)
        c["metallic"] = np.where(np.arange(n) % 3 == 1, np.float32(1.0), c["metallic"]).astype(np.float32)
        return c, None
    raise KeyError(kind)


def _queue(dirs, ws, keep, kinds=None):
    """per-sample lists ([c, n] planes, [n] masks) -> dict of the flattened point-major queue and the offsets"""
    keep = np.stack(keep, axis=1)                                   # [n, spp]
    n, spp = keep.shape
    sel = keep.reshape(-1)
    flat = lambda a: np.stack(a, axis=2).reshape(a[0].shape[0], -1)[:, sel]     # [c, n*spp] point-major -> kept
    pts, smp = np.meshgrid(np.arange(n), np.arange(spp), indexing="ij")
    q = dict(dir=flat(dirs), weight=flat(ws), point=pts.reshape(-1)[sel], sample=smp.reshape(-1)[sel],
             offsets=np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64))
    if kinds is not None:
        q["kind"] = np.stack(kinds, axis=1).reshape(-1)[sel]
    return q


def ggx_oracle_queue(case, exiting, spp_n, seed, refract, first=0):
    """the rlGgx queue composed on the CPU: per sample s the scrambled (0,2) point (orc_sample_02, dim pair 0), the oracle
    closure's evalSample / evalBrdf / evalPdf (glossy: weight f/pdf) or refract sample (weight, refracted flag); kept unless
    the weight is zero.  -> dict of the flattened point-major queue and the offsets"""
    from gpu_util import ggx_oracle
    n, spp = case["wo"].shape[1], spp_n * spp_n
    og = ggx_oracle(O, case, exiting=exiting)
    dirs, ws, keep, kinds = [], [], [], []
    for s in range(spp):
        rx, ry = O.batch_sample_02(seed, first, n, 0, s)
        if refract:
            wt, w, flag = og.refract(rx, ry)
            dirs.append(wt); ws.append(w[None, :]); keep.append(w != 0.0); kinds.append(np.where(flag != 0, 0, 1))
        else:
            wi, f, pdf, _ = og.sample_eval_pdf(rx, ry)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                t = (f / pdf[None, :]).astype(np.float32)
            dirs.append(wi); ws.append(t); keep.append(~np.all(t == 0.0, axis=0)); kinds.append(np.zeros(n, np.int64))
    return _queue(dirs, ws, keep, kinds)


def disney_oracle_queue(case, spp_n, seed, lobe, first=0):
    """the rlDisney queue of one lobe composed on the CPU: per sample s the scrambled (0,2) point (orc_sample_02, dimension
    pair 0 for the diffuse lobe, 1 for the specular one) and the oracle closure's sample / eval / pdf triple for the lobe;
    kept where pdf > 1e-4 and f / pdf is not all zero -> dict of the flattened point-major queue and the offsets"""
    from gpu_util import disney_oracle
    n, spp = case["wo"].shape[1], spp_n * spp_n
    od = disney_oracle(O, case)
    pair = 0 if lobe == DIFFUSE else 1
    dirs, ws, keep = [], [], []
    for s in range(spp):
        rx, ry = O.batch_sample_02(seed, first, n, pair, s)
        wi, f, pdf = od.sample_eval_pdf(lobe, rx, ry)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t = (f / pdf[None, :]).astype(np.float32)
        dirs.append(wi); ws.append(t); keep.append((pdf > EPS) & ~np.all(t == 0.0, axis=0))
    return _queue(dirs, ws, keep)


def radiance(d, k):
    """a deterministic float32 sky: a function of the direction and of the ray index"""
    d = d.astype(np.float32)
    k = k.astype(np.float32)
    r = np.float32(0.25) + np.float32(0.75) * np.maximum(d[2], np.float32(0.0))
    g = np.float32(1.0) + np.float32(0.5) * d[0] * d[1]
    b = np.float32(0.5) + np.float32(1e-3) * np.mod(k, np.float32(97.0))
    return np.stack([r, g, b]).astype(np.float32)


def sequential(L, w, offsets, inv=None):
    """float32 sum per point over its rays in queue order (sum += L * w), times inv afterwards"""
    n = len(offsets) - 1
    cnt = np.diff(offsets)
    acc = np.zeros((3, n), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (L * w).astype(np.float32)
        for j in range(int(cnt.max()) if n else 0):
            m = cnt > j
            acc[:, m] = acc[:, m] + prod[:, offsets[:-1][m] + j]
        if inv is not None:
            acc = acc * np.float32(inv)
    return acc
