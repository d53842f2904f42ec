"""GPU: the one-sample ("pointwise") verbs past one tile per workgroup, at tile, round and plane edges (tests/pointwise_util.py).

Every pointwise kernel hoists parameter-only arithmetic (UNIFORM_* modes), takes `tile_range(n)` and walks one tile per loop
iteration.  On the default context no affordable size reaches the second iteration, so a context capped at one workgroup per CU
(RLS_BLOCKS_PER_CU=1) runs n_A = 2.5 x cu x 256 + 77 points (plain cap, hoisting grid) and n_B = 16 x that + 77 (the rlGgx and rlSkin
per-point launches): every workgroup walks two or three tiles, an XCD's eighth is short, the batch ends in a 77-point tile
(pointwise_util.check_sizes proves it from a restatement of grid_for / grid_for_hoisting / tile_range; the clock stamps tie the
restatement to the library).  Between two device runs the gate is 0 differing words, NaN equal to NaN by bit pattern, no point
excluded; against the oracle the gates of each verb's own parity test (tests/cases.py), on 512-point windows around the round
boundaries of the first and last XCD and around the final partial tile.

  rounds      every verb, STREAMED and MIXED: capped context = default context (one tile per workgroup) = oracle on the windows;
  hoisted     the UNIFORM specialisations: capped = default = the STREAMED kernel on the same values as planes = oracle;
  reference   materials=(ids, 37) on the capped context = the expanded planes on the default one;
  small n     n = 1 .. 9 x 256 + 1 against the oracle: partial wavefronts, the first grid of 8, empty per-XCD eighths;
  sentinels   nothing but the n words of each output plane is written, every one of them is;
  FAST        the FAST kernels give the same words on the capped and the default context."""
import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
import pointwise_util as U
from test_gpu_uniform_parameters import DISNEY_DEFAULTS, DISNEY_UNIFORM, GGX_UNIFORM
from test_gpu_sss_skin import SKIN_UNIFORM_CASES, UNIFORM_DISTANCES

pytestmark = pytest.mark.gpu

UNITS = ("ggx", "disney", "alt", "gauss", "sss", "misc", "skin")


@pytest.fixture(scope="module")
def capped(gpu):
    ctx = U.capped_context()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def fast_pair(gpu):
    a, b = U.capped_context(fast=True), R.Context(0)
    b.set_math_mode(True)
    yield a, b
    a.close()
    b.close()


@pytest.fixture(scope="module")
def sizes(gpu):
    """{"A": n_A, "B": n_B, "cu", "grid": the capped context's grids}, with the restatement's proof that the loop iterates"""
    cu = gpu.device_info()["compute_units"]
    print("sizes", U.check_sizes(cu))
    return {"A": U.n_a(cu), "B": U.n_b(cu), "cu": cu, "grid": U.capped_grids(cu)}


def _windows(sizes, verb):
    return U.boundary_windows(sizes["grid"][verb.size], sizes[verb.size])


def test_restated_grids_are_the_library_s(gpu, capped, sizes):
    """the clock stamps count the workgroups of a stamped launch: grid_for at cap_mult 16 (streamed reflect+refract, streamed
    rlSkin) and at cap_mult 1 (the per-point rlSss probe), on both contexts; the stamped reflect+refract is the frozen
    ggx_kernel<5, 0, 1>, so its capped result is compared with the default context's too"""
    V = U._build_verbs()
    cu = sizes["cu"]
    res = {}
    for ctx, bpc in ((capped, 1), (gpu, U.DEFAULT_BLOCKS_PER_CU)):
        for name, cap_mult in (("ggx.reflectRefract", U.CAP_MULT), ("skin.sampleEvalPdf", U.CAP_MULT), ("sss.probe.dPdu", 1)):
            v = V[name]
            n = sizes[v.size]
            I, P = U.inputs(gpu, v.unit, n)
            got = []
            grid = U.stamped_grid(ctx, lambda: got.extend(U.run(ctx, v, I, P)))
            assert grid == U.grid_for(cu, bpc, n, cap_mult), (name, bpc, grid)
            res[name, bpc] = got
    for name in ("ggx.reflectRefract", "skin.sampleEvalPdf", "sss.probe.dPdu"):
        assert U.differing(res[name, 1], res[name, U.DEFAULT_BLOCKS_PER_CU]) == 0, name
    assert U.grid_for_hoisting(cu, 1, sizes["A"]) == sizes["grid"]["A"]          # (no stamped launch: the restatement alone)


# ---- 1. rounds, per-point modes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", UNITS)
def test_rounds_per_point_modes(gpu, capped, sizes, unit):
    V = U._build_verbs()
    for name in U.verb_names(unit):
        v = V[name]
        n = sizes[v.size]
        I, P0 = U.inputs(gpu, v.unit, n)
        for mode in U.modes(v):
            P = U.with_mode(v, P0, mode)
            got, base = U.run(capped, v, I, P), U.run(gpu, v, I, P)
            d = U.differing(got, base)
            print(name, mode, "n", n, "words differing between the capped and the default context:", d)
            assert d == 0, (name, mode, d)
            U.check_windows(v, got, I, P, _windows(sizes, v), n, mode)


# ---- 2. rounds, hoisted modes ------------------------------------------------------------------------------------------------------
def _uniform_sets(sizes):
    """(verb name, tag, uniform parameters or a callable of the per-point planes) of every UNIFORM specialisation"""
    out = []
    for name in U.verb_names("ggx"):
        for tag in ("plastic", "brushed"):                                       # brushed: ior < 1
            p = GGX_UNIFORM[tag]
            for cmap in (False, True):                                           # specColor uniform / textured
                out.append((name, f"{tag}{'+map' if cmap else ''}", dict(p), "KsColor" if cmap else None))
    for name in U.verb_names("disney"):
        for tag in ("every_lobe", "extremes"):
            for cmap in (False, True):                                           # UNIFORM_ALL / UNIFORM_SCALARS
                out.append((name, f"{tag}{'+map' if cmap else ''}", dict(DISNEY_DEFAULTS, **DISNEY_UNIFORM[tag]),
                            "base_color" if cmap else None))
    for name in ("sss.probe.dPdu", "sss.probe.polar", "sss.nd_sample", "sss.nd_pdf", "sss.mis_pdf"):
        for dist, mult in ((UNIFORM_DISTANCES[0], None), (UNIFORM_DISTANCES[4], 1.7)):
            out.append((name, f"{dist}x{mult}", dict(dist=dist, multiplier=mult, albedo=(0.8, 0.5, 0.4)), None))
    for tag in ("all_layers", "no_sheen"):                                       # no_sheen: one layer weight 0
        out.append(("skin.sampleEvalPdf", tag, dict(SKIN_UNIFORM_CASES[tag]), None))
    return out


def _uniform_arms(gen, ctx_capped, ctx_default, sizes, unit, streamed_arm=True, oracle_arm=True):
    V = U._build_verbs()
    ran = 0
    for name, tag, p, map_key in _uniform_sets(sizes):
        v = V[name]
        if v.unit != unit:
            continue
        n = sizes["A"]                                                           # grid_for_hoisting: the plain cap for every unit
        I, P0 = U.inputs(gen, v.unit, n)
        P = dict(p)
        if map_key:
            P[map_key] = P0[map_key]
        got = U.run(ctx_capped, v, I, P)
        d = U.differing(got, U.run(ctx_default, v, I, P))                        # (a) one tile per workgroup
        print(name, tag, "words differing, capped vs default context:", d)
        assert d == 0, (name, tag, "capped vs default context", d)
        if streamed_arm:                                                         # (b) the STREAMED kernel on the same values
            d = U.differing(got, U.run(ctx_default, v, I, U.as_planes(P, n)))
            assert d == 0, (name, tag, "capped UNIFORM vs STREAMED on the default context", d)
        if oracle_arm:                                                           # (c) the oracle on the boundary windows
            wins = U.boundary_windows(sizes["grid"]["A"], n)
            hI, hP, idx = U.host_window(I, P, wins, n)
            ref = v.ref(hI, hP)
            kinds = U.bit_gates(v) if cases.strict_parity() else v.gates
            for (pl, _, _), kind, g, r in zip(v.planes, kinds, got, ref):
                g = g[..., idx].contiguous().cpu().numpy()
                if kind == "b":                                                  # NaN equal to NaN, as the uniform tests hold it
                    g, r = np.ascontiguousarray(g), np.ascontiguousarray(r, dtype=np.float32)
                    ok = (g.view(np.uint32) == r.view(np.uint32)) | (np.isnan(g) & np.isnan(r))
                    assert ok.all(), (name, tag, pl, "vs oracle", int((~ok).sum()))
                else:
                    U.gate(kind, g, r, (name, tag, pl))
        ran += 1
    assert ran > 0


@pytest.mark.parametrize("unit", ["ggx", "disney", "sss", "skin"])
def test_rounds_hoisted_modes(gpu, capped, sizes, unit):
    _uniform_arms(gpu, capped, gpu, sizes, unit)


# ---- 3. by reference across rounds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ggx.reflectRefract", "disney.sampleEvalPdf.diffuse", "disney.sampleEvalPdf.glossy",
                                  "sss.probe.dPdu", "skin.sampleEvalPdf"])
def test_by_reference_across_rounds(gpu, capped, sizes, name):
    v = U._build_verbs()[name]
    n = sizes[v.size]
    I, _ = U.inputs(gpu, v.unit, n)
    ids, cols, planes = U.material_columns(gpu, v.unit, n)
    got = U.run(capped, v, I, cols, mat=(ids, U.M))
    d = U.differing(got, U.run(gpu, v, I, planes))
    assert d == 0, (name, d)


# ---- 4. tile_range at small n ------------------------------------------------------------------------------------------------------
MAIN = ("ggx.sampleEvalPdf", "disney.sampleEvalPdf.glossy", "sss.probe.dPdu", "skin.sampleEvalPdf", "sss.nd_sample")
MAIN_UNIFORM = {"ggx.sampleEvalPdf": dict(GGX_UNIFORM["plastic"]),
                "disney.sampleEvalPdf.glossy": dict(DISNEY_DEFAULTS, **DISNEY_UNIFORM["every_lobe"]),
                "sss.probe.dPdu": dict(dist=UNIFORM_DISTANCES[0], multiplier=None, albedo=(0.8, 0.5, 0.4)),
                "sss.nd_sample": dict(dist=UNIFORM_DISTANCES[0], multiplier=None, albedo=(0.8, 0.5, 0.4)),
                "skin.sampleEvalPdf": dict(SKIN_UNIFORM_CASES["all_layers"])}


def _small(gpu, name, n, uniform):
    v = U._build_verbs()[name]
    I, P = U.inputs(gpu, v.unit, n, layers_on=True)       # rlSkin: sheen and specular on at every point
    if uniform:
        P = MAIN_UNIFORM[name]
    return v, I, P, U.run(gpu, v, I, P)


@pytest.mark.parametrize("n", U.SMALL_SIZES)
def test_tile_range_at_small_n(gpu, n):
    for name in MAIN:
        for uniform in (False, True):
            v, I, P, got = _small(gpu, name, n, uniform)
            U.check_windows(v, got, I, P, None, n, ("UNIFORM" if uniform else "STREAMED", n))


@pytest.mark.parametrize("n", [65, 255])
def test_whole_wavefronts_of_a_partial_tile_carry_the_full_tile_s_bits(gpu, n):
    """the first 64 x floor(n / 64) points at n = 65 and 255 = the n = 256 run of the same inputs (the generators are
    counter-based: n points are the first n of 256); rlSkin's full wavefronts take the ballot == ~0 path in both runs, the
    partial one the general path"""
    keep = n // 64 * 64
    for name in MAIN:
        for uniform in (False, True):
            _, _, _, part = _small(gpu, name, n, uniform)
            _, _, _, full = _small(gpu, name, 256, uniform)
            d = U.differing([t[..., :keep].contiguous() for t in part], [t[..., :keep].contiguous() for t in full])
            assert d == 0, (name, uniform, n, d)


# ---- 5. nothing beside the planes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 513, "n_A"])
@pytest.mark.parametrize("unit", UNITS)
def test_output_planes_leave_the_words_beside_them(gpu, capped, sizes, unit, n):
    V = U._build_verbs()
    ctx = gpu
    if n == "n_A":                            # the capped context: the last round's partial tile is a grid-stride iteration
        n, ctx = sizes["A"], capped
    for name in U.verb_names(unit):
        v = V[name]
        I, P0 = U.inputs(gpu, v.unit, n)
        for mode in U.modes(v):
            P = U.with_mode(v, P0, mode)
            if mode == "STREAMED":            # these inputs never yield the sentinel's payload: the oracle says so first
                hI, hP, _ = U.host_window(I, P, None, n)
                U.oracle_never_yields_the_sentinel(v.ref(hI, hP))
            plain = U.run(ctx, v, I, P)
            bufs, views = U.sentinel_out(v, n)
            got = U.run(ctx, v, I, P, out=views)
            assert U.differing([g.contiguous() for g in got], plain) == 0, (name, mode, n)
            U.check_sentinels(v, bufs, n, (mode, n))


# ---- 6. the FAST flavour -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", UNITS)
def test_fast_kernels_across_rounds(gpu, fast_pair, sizes, unit):
    """FAST kernels, capped against default context: the same words (their accuracy is test_gpu_fast_mode.py's business)"""
    fc, fd = fast_pair
    V = U._build_verbs()
    for name in U.verb_names(unit):
        v = V[name]
        n = sizes[v.size]
        I, P0 = U.inputs(gpu, v.unit, n)
        for mode in U.modes(v):
            P = U.with_mode(v, P0, mode)
            d = U.differing(U.run(fc, v, I, P), U.run(fd, v, I, P))
            assert d == 0, (name, mode, "FAST", d)
    if unit in ("ggx", "disney", "sss", "skin"):
        _uniform_arms(gpu, fc, fd, sizes, unit, streamed_arm=False, oracle_arm=False)
