"""Helper of tests/test_gpu_pointwise_edges.py: the one-sample ("pointwise") verbs of the product library past one tile per
workgroup.

Every pointwise kernel (ggx_kernel, disney_kernel, sss_kernel, misc_kernel, skin_kernel, alt_kernel) runs one skeleton:
parameter-only arithmetic hoisted ahead of the loop (UNIFORM_* modes), `tiles = tile_range(n)`, then one iteration per tile.
The host sizes the grid with grid_for(ctx, n, kBlock, cap_mult) or grid_for_hoisting(ctx, n) (csrc/rls_internal.hpp).  On the
default context no size a test can afford reaches the loop's second iteration, so the tests use a context capped at one
workgroup per CU (RLS_BLOCKS_PER_CU=1, read per context) and the two sizes of `n_a` / `n_b` below.

The first part of this module restates grid_for, grid_for_hoisting and tile_range in plain Python (no device, no torch):
`check_sizes(cu)` proves from the restatement that at the chosen sizes every workgroup that owns a tile walks at least two and
some walk three, that an XCD has a short eighth and that the batch ends in a partial tile
(`python tests/pointwise_util.py --check-sizes 256`).  The restatement of grid_for is tied to the library where the library
reports its grid: the clock stamps of a streamed reflect+refract or rlSkin launch (cap_mult 16) and of a per-point rlSss probe
(cap_mult 1) count the workgroups (`stamped_grid`).  grid_for_hoisting has no stamped launch: its restatement stands alone,
checked against the source by reading only.

The second part holds the inputs (generated on the device by the library's seeded generators, the distributions of
tests/cases.py), the table of verbs (`VERBS`: how to run one, its output planes, its oracle call and the gate its existing parity
test applies per plane) and the comparisons: `differing` counts differing words on the device (NaN equal to NaN by bit
pattern, no point excluded); `check_windows` runs the oracle on 512-point windows around the round boundaries."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
TILE = 256                       # rlsh::kBlock
CAP_MULT = 16                    # RLS_CAP_MULT: the rlGgx and rlSkin per-point launches
DEFAULT_BLOCKS_PER_CU = 64       # rls_context_create
HOIST_TILES_PER_THREAD = 8       # RLS_HOIST_TILES_PER_THREAD
HOIST_MIN_BLOCKS_PER_CU = 16     # RLS_HOIST_MIN_BLOCKS_PER_CU
SMALL_SIZES = (1, 63, 64, 65, 255, 256, 257, 7 * 256, 7 * 256 + 1, 8 * 256 + 1, 9 * 256 + 1)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _round8(want):
    return (want + 7) // 8 * 8 if want >= 8 else want


def grid_for(cu, blocks_per_cu, n, cap_mult=1, points_per_block=TILE):
    want = (n + points_per_block - 1) // points_per_block
    want = min(max(want, 1), cu * blocks_per_cu * cap_mult)
    return _round8(want)


def grid_for_hoisting(cu, blocks_per_cu, n, points_per_block=TILE):
    tiles = (n + points_per_block - 1) // points_per_block
    want = (tiles + HOIST_TILES_PER_THREAD - 1) // HOIST_TILES_PER_THREAD
    want = max(want, cu * HOIST_MIN_BLOCKS_PER_CU)
    want = min(want, cu * blocks_per_cu)
    want = max(min(want, tiles), 1)
    return _round8(want)


def tile_range(grid, block, n):
    """(first, end, step) in points of workgroup `block` of a grid of `grid`"""
    if grid % 8 == 0:
        tiles = (n + TILE - 1) // TILE
        per_xcd = (tiles + 7) // 8
        x, b = block % 8, block // 8
        return (x * per_xcd + b) * TILE, min((x + 1) * per_xcd * TILE, n), grid // 8 * TILE
    return block * TILE, n, grid * TILE


def tiles_per_workgroup(grid, n):
    return [len(range(*tile_range(grid, b, n))) for b in range(grid)]


def covered_once(grid, n):
    """every tile of the batch is walked by exactly one workgroup"""
    seen = sorted(base for b in range(grid) for base in range(*tile_range(grid, b, n)))
    return seen == list(range(0, n, TILE))


def n_a(cu):
    """2.5 x cu x 256 + 77: for every launch under the plain cap (grid_for(ctx, n)) and every grid_for_hoisting launch"""
    return 640 * cu + 77


def n_b(cu):
    """2.5 x cu x 16 x 256 + 77: for the per-point rlGgx and rlSkin launches (cap_mult 16); rr_wg_util.ROUNDS_N at cu = 256"""
    return 640 * CAP_MULT * cu + 77


def capped_grids(cu):
    """{size: grid} of the context capped at one workgroup per CU"""
    return {"A": grid_for(cu, 1, n_a(cu)), "B": grid_for(cu, 1, n_b(cu), CAP_MULT)}


def boundary_windows(grid, n, width=512):
    """[(first, end)]: `width` points around every round boundary of the first and the last XCD's eighth (of every round of a
    grid that is no multiple of 8), and the last `width` points: the final partial tile and the tile before it"""
    tiles = (n + TILE - 1) // TILE
    bounds = []
    if grid % 8 == 0:
        per_xcd, step = (tiles + 7) // 8, grid // 8
        for x in (0, 7):
            bounds += [t * TILE for t in range(x * per_xcd + step, min((x + 1) * per_xcd, tiles), step)]
    else:
        bounds = [t * TILE for t in range(grid, tiles, grid)]
    wins = {(max(0, p - width // 2), min(n, p + width // 2)) for p in bounds}
    wins.add((max(0, n - width), n))
    return sorted(wins)


def check_sizes(cu):
    """the assertions the issue of this file asks of the chosen sizes, from the restatement alone"""
    report = {}
    na, nb = n_a(cu), n_b(cu)
    for what, n, grid in (("grid_for, cap_mult 1", na, grid_for(cu, 1, na)),
                          ("grid_for_hoisting", na, grid_for_hoisting(cu, 1, na)),
                          ("grid_for, cap_mult 16", nb, grid_for(cu, 1, nb, CAP_MULT))):
        per = tiles_per_workgroup(grid, n)
        busy = [t for t in per if t]
        assert covered_once(grid, n), (what, "a tile is walked twice or never")
        assert busy and min(busy) >= 2, (what, "a workgroup walks one tile only", min(busy))
        assert max(busy) >= 3 and min(busy) == 2, (what, "no mix of two and three rounds", min(busy), max(busy))
        assert n % TILE == 77, (what, "the batch must end in a 77-point tile")
        tiles = (n + TILE - 1) // TILE
        short = None
        if grid % 8 == 0:
            per_xcd = (tiles + 7) // 8
            short = tiles - 7 * per_xcd
            assert 0 < short < per_xcd, (what, "the last XCD's eighth is not short", short, per_xcd)
            assert per_xcd % (grid // 8) != 0, (what, "per_xcd is a multiple of the per-XCD step")
        assert len(boundary_windows(grid, n)) >= 3
        report[what] = dict(n=n, tiles=tiles, grid=grid, rounds=(min(busy), max(busy)), last_eighth=short)
    # on the default context the same sizes are one tile per workgroup: the arm the capped one is compared with
    for n, grid in ((na, grid_for(cu, DEFAULT_BLOCKS_PER_CU, na)), (na, grid_for_hoisting(cu, DEFAULT_BLOCKS_PER_CU, na)),
                    (nb, grid_for(cu, DEFAULT_BLOCKS_PER_CU, nb, CAP_MULT))):
        assert max(tiles_per_workgroup(grid, n)) == 1 and covered_once(grid, n), (n, grid)
    # the small sizes of the tile_range test: the first grid of 8 and the first with empty eighths
    assert grid_for(cu, DEFAULT_BLOCKS_PER_CU, 7 * 256 + 1) == 8 and tiles_per_workgroup(8, 7 * 256 + 1) == [1] * 8
    g = grid_for(cu, DEFAULT_BLOCKS_PER_CU, 8 * 256 + 1)
    per = tiles_per_workgroup(g, 8 * 256 + 1)
    assert g == 16 and all(per[b] == 0 for b in range(16) if b % 8 >= 5) and sum(per) == 9, (g, per)
    for n in SMALL_SIZES:
        for g in (grid_for(cu, DEFAULT_BLOCKS_PER_CU, n), grid_for_hoisting(cu, DEFAULT_BLOCKS_PER_CU, n)):
            assert covered_once(g, n), (n, g)
    return report


# ---- the device side ---------------------------------------------------------------------------------------------------------------
SEED = 99                        # cases.SEED_PARITY
SENTINEL = 0x7FC0DEAD            # a quiet NaN with a payload: no kernel writes it
BYTE_SENTINEL = 0xA5
PAD = 67
M = 37                           # node instances of the by-reference batches
torch = R = O = cases = None


def _need():
    global torch, R, O, cases
    if torch is None:
        for p in (str(ROOT), str(ROOT / "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        import torch as _t
        import rlshaders_amd as _r
        import oracle_lib as _o
        import cases as _c
        torch, R, O, cases = _t, _r, _o, _c


def capped_context(fast=False):
    """a context whose grid cap is one workgroup per CU; the variable is read per context, so only its creation sees it"""
    _need()
    import pytest
    mp = pytest.MonkeyPatch()
    mp.setenv("RLS_BLOCKS_PER_CU", "1")
    try:
        ctx = R.Context(0)
    finally:
        mp.undo()
    if fast:
        ctx.set_math_mode(True)
    return ctx


def stamped_grid(ctx, launch):
    """workgroups of the stamped launch `launch()` enqueues (0: it has no stamped instantiation)"""
    ctx.clock_stamps_begin()
    try:
        launch()
        return len(ctx.clock_stamps_read())
    finally:
        ctx.clock_stamps_end()


def differing(a, b):
    """words (bytes of a byte plane) that differ between two lists of device planes, NaN equal to NaN by bit pattern"""
    d = 0
    for p, q in zip(a, b):
        assert p.shape == q.shape and p.dtype == q.dtype, (p.shape, q.shape, p.dtype, q.dtype)
        if p.dtype == torch.float32:
            p, q = p.view(torch.int32), q.view(torch.int32)
        d += int((p != q).sum())
    return d


# inputs: device tensors, the distributions of cases.ggx_mixed / disney_mixed / sss_mixed / skin_mixed (the same seeded streams)
_CACHE = {}


def _u(ctx, n, stream, lo=0.0, hi=1.0, seed=SEED):
    return R.gen_uniform(ctx, seed, 0, n, stream, lo, hi)


def _u3(ctx, n, stream, lo=0.0, hi=1.0, seed=SEED):
    return torch.stack([_u(ctx, n, stream + j, lo, hi, seed) for j in range(3)])


def _ggx_params(ctx, m, seed=SEED):
    return dict(KsColor=_u3(ctx, m, O.S_KS_R, seed=seed), roughness=_u(ctx, m, O.S_ROUGH, 0.05, 1.0, seed),
                ior=_u(ctx, m, O.S_IOR, 1.05, 2.55, seed), anisotropic=R.gen_aniso(ctx, seed, 0, m))


def _disney_params(ctx, m, seed=SEED):
    p = dict(base_color=_u3(ctx, m, O.S_KS_R, seed=seed))
    for k, name in enumerate(O.DISNEY_SCALARS):
        p[name] = _u(ctx, m, O.S_PARAM0 + k, seed=seed)
    return p


def _sss_params(ctx, m, seed=SEED):
    return dict(dist=_u3(ctx, m, O.S_PARAM0, 0.1, 2.1, seed), albedo=_u3(ctx, m, O.S_KS_R, seed=seed),
                multiplier=_u(ctx, m, O.S_PARAM0 + 4, 0.5, 1.5, seed))


def _skin_params(ctx, m, seed=SEED, layers_on=False):
    u = lambda k, lo=0.0, hi=1.0: _u(ctx, m, O.S_PARAM0 + k, lo, hi, seed)
    u3 = lambda k, lo=0.0, hi=1.0: _u3(ctx, m, O.S_PARAM0 + k, lo, hi, seed)
    w = (0.2, 1.0) if layers_on else (0.0, 1.0)       # layers_on: sheen and specular evaluated at every point
    return dict(sss_color=u3(0), sss_weight=u(3), sss_dist_multiplier=u(4, 0.5, 1.5), sss_scatter_dist=u3(5, 0.1, 2.1),
                specular_color=u3(8), specular_weight=u(11, *w), specular_roughness=u(12, 0.05, 1.0), specular_ior=u(13, 1.05, 2.55),
                sheen_color=u3(14), sheen_weight=u(17, *w), sheen_roughness=u(18, 0.05, 1.0), sheen_ior=u(19, 1.05, 2.55))


PARAMS = {"ggx": _ggx_params, "disney": _disney_params, "alt": _disney_params, "sss": _sss_params, "misc": lambda ctx, m, seed=SEED: {},
          "gauss": lambda ctx, m, seed=SEED: dict(dist_x=_u(ctx, m, O.S_PARAM0, 0.1, 2.1, seed)), "skin": _skin_params}
# MIXED: one scalar parameter a plain value, the rest planes
MIXED = {"ggx": dict(roughness=0.35), "disney": dict(roughness=0.4), "alt": dict(roughness=0.4), "sss": dict(multiplier=1.7),
         "gauss": dict(dist_x=1.5), "skin": dict(sheen_roughness=0.35)}


def inputs(ctx, unit, n, layers_on=False):
    """(I, P): the per-point inputs and the per-point parameter planes of `unit` at n points, made once per (unit, n)"""
    _need()
    key = (unit, n, layers_on)
    if key in _CACHE:
        return _CACHE[key]
    wo, N, T = R.gen_frame(ctx, SEED, 0, n)
    I = dict(wo=wo, N=N, T=T, x=torch.stack([_u(ctx, n, O.S_XI0 + j) for j in range(6)]))
    P = PARAMS[unit](ctx, n) if unit != "skin" else _skin_params(ctx, n, layers_on=layers_on)
    if unit == "ggx":
        I["exiting"] = (torch.arange(n, device="cuda") % 3 == 0).to(torch.uint8)
        I["indir"] = _ggx(ctx, I, P).sampleEvalPdf(I["x"][0], I["x"][1])[0]
    elif unit in ("disney", "alt"):
        s = _disney(ctx, I, P)
        I["indir"] = s.sampleEvalPdf(I["x"][0], I["x"][1])[0]          # the glossy lobe's sampled direction
    elif unit in ("sss", "misc"):
        I["Tu"] = (T * 2.5 + 0.3 * N).contiguous()                     # dPdu: scaled, not orthogonal to N (Gram-Schmidt frame)
        I["r"] = _u(ctx, n, O.S_XI0 + 7, 0.01, 2.0)
        I["disp"] = (_u3(ctx, n, O.S_XI0 + 8) - 0.5).contiguous()
        I["sN"] = R.gen_frame(ctx, 7, 0, n)[1]
        I["i"] = (_u3(ctx, n, O.S_XI0 + 11) * 2 - 1).contiguous()
        I["col"] = _u3(ctx, n, O.S_XI0 + 14)
    torch.cuda.synchronize()
    _CACHE[key] = (I, P)
    return I, P


def material_columns(ctx, unit, n):
    """(ids int32 [n], columns of M entries, the columns expanded into per-point planes)"""
    _need()
    g = torch.Generator(device="cpu").manual_seed(5)
    ids = torch.randint(0, M, (n,), generator=g, dtype=torch.int32)
    ids[:M] = torch.arange(M, dtype=torch.int32)                    # every material occurs
    ids = ids.cuda()
    cols = PARAMS[unit](ctx, M, seed=7)
    if unit == "ggx":
        cols["ior"][::5] = 0.7                                      # some instances below 1
    if unit == "skin":
        cols["sheen_weight"][::4] = 0.0                             # layers off in some instances
    planes = {k: v[..., ids.long()].contiguous() for k, v in cols.items()}
    return ids, cols, planes


def as_planes(P, n):
    """uniform values -> the same values as per-point planes (the float32 a C float parameter holds)"""
    out = {}
    for k, v in P.items():
        if torch.is_tensor(v) or v is None:
            out[k] = v
        elif isinstance(v, (tuple, list)):
            out[k] = torch.tensor([float(c) for c in v], dtype=torch.float32, device="cuda").reshape(3, 1).expand(3, n).contiguous()
        else:
            out[k] = torch.full((n,), float(v), dtype=torch.float32, device="cuda")
    return out


# ---- the verbs ---------------------------------------------------------------------------------------------------------------------
def _ggx(ctx, I, P, mat=None):
    return R.GgxSampler(ctx, I["wo"], I["N"], I["T"], specColor=P["KsColor"], ior=P["ior"], roughness=P["roughness"],
                        anisotropic=P["anisotropic"], exiting=I.get("exiting"), materials=mat)


def _disney(ctx, I, P, mat=None, lobe=None):
    s = R.DisneySampler(ctx, I["wo"], I["N"], I["T"], materials=mat, **P)
    if lobe is not None:
        s.setSampleType(lobe)
    return s


def _nd(ctx, I, P, mat=None):
    kw = {} if P.get("multiplier") is None else dict(multiplier=P["multiplier"])
    return R.NDProfile(ctx, I["x"].shape[-1], P["dist"], P["albedo"], materials=mat, **kw)


def _sss(ctx, I, P, mat=None, dpdu=True):
    kw = {} if P.get("multiplier") is None else dict(multiplier=P["multiplier"])
    return R.SssSampler(ctx, I["N"], I["Tu"] if dpdu else I["T"], P["albedo"], P["dist"], has_dPdu=dpdu, materials=mat, **kw)


def _oggx(h, P):
    g = O.Ggx(h["wo"], h["N"], h["T"], KsColor=P["KsColor"], ior=P["ior"], roughness=P["roughness"], anisotropic=P["anisotropic"],
              exiting=h.get("exiting"), nthreads=4)
    g.two_sums_default = True
    return g


def _odisney(h, P):
    return O.Disney(h["wo"], h["N"], h["T"], nthreads=4, **P)


def _osss(h, P, dpdu=None):
    n = h["x"].shape[-1]
    if dpdu is None:
        return O.Sss(n, P["dist"], P["albedo"], multiplier=P.get("multiplier"), nthreads=4)
    return O.Sss(n, P["dist"], P["albedo"], multiplier=P.get("multiplier"), N=h["N"], T=h["Tu"] if dpdu else h["T"], has_dPdu=dpdu,
                 nthreads=4)


PROBE_KEYS = ("r", "origin", "dir", "maxdist", "pdf", "profile")
PROBE_PLANES = [("r", 1, "f"), ("origin", 3, "f"), ("dir", 3, "f"), ("maxdist", 1, "f"), ("pdf", 1, "f"), ("profile", 3, "f")]
SKIN_KEYS = ("sheen_wi", "sheen_f", "sheen_pdf", "sheen_fresnel", "spec_wi", "spec_f", "spec_pdf", "spec_fresnel",
             "r", "r_pdf", "profile", "sheenFresnel", "specularFresnel", "sssWeight")
SKIN_PLANES = [(k, 3 if k in ("sheen_wi", "sheen_f", "spec_wi", "spec_f", "profile") else 1, "f") for k in SKIN_KEYS]


def _dict_out(keys, out):
    return None if out is None else dict(zip(keys, out))


def _one(t):
    return [t]


class Verb:
    """unit: whose parameters it takes; size: "A" (plain cap / hoisting grid) or "B" (cap_mult 16); planes: (name, rows, "f" |
    "b"); run(ctx, I, P, out, mat) -> list of device planes; ref(h, P) -> the oracle's; gates: per plane, "t" cases.assert_tight,
    "l" every point within 1e-5, "b" the same bits, "f" flags (cases.flag_slack)"""

    def __init__(self, name, unit, size, planes, run, ref, gates):
        self.name, self.unit, self.size, self.planes, self.run, self.ref, self.gates = name, unit, size, planes, run, ref, gates
        assert len(gates) == len(planes), name


V3, V1 = lambda nm: (nm, 3, "f"), lambda nm: (nm, 1, "f")
X = lambda I, k: I["x"][k]
_t = lambda out, k: None if out is None else out[k]
VERBS = {}


def _add(*a):
    VERBS[a[0]] = Verb(*a)


def _build_verbs():
    _need()
    if VERBS:
        return VERBS
    _add("ggx.evalSample", "ggx", "B", [V3("wi"), V1("fresnel")],
         lambda c, I, P, o, m: list(_ggx(c, I, P, m).evalSample(X(I, 0), X(I, 1), _t(o, 0), _t(o, 1))),
         lambda h, P: _oggx(h, P).sample(h["x"][0], h["x"][1]), "tt")
    _add("ggx.sampleEvalPdf", "ggx", "B", [V3("wi"), V3("f"), V1("pdf"), V1("fresnel")],
         lambda c, I, P, o, m: list(_ggx(c, I, P, m).sampleEvalPdf(X(I, 0), X(I, 1), out=o)),
         lambda h, P: _oggx(h, P).sample_eval_pdf(h["x"][0], h["x"][1]), "tttt")
    _add("ggx.evalBrdf", "ggx", "B", [V3("f")], lambda c, I, P, o, m: _one(_ggx(c, I, P, m).evalBrdf(I["indir"], out=_t(o, 0))),
         lambda h, P: _one(_oggx(h, P).eval(h["indir"])), "l")
    _add("ggx.evalPdf", "ggx", "B", [V1("pdf")], lambda c, I, P, o, m: _one(_ggx(c, I, P, m).evalPdf(I["indir"], out=_t(o, 0))),
         lambda h, P: _one(_oggx(h, P).pdf(h["indir"])), "l")
    _add("ggx.ndfPdf", "ggx", "B", [V1("pdf")], lambda c, I, P, o, m: _one(_ggx(c, I, P, m).ndfPdf(I["indir"], out=_t(o, 0))),
         lambda h, P: _one(_oggx(h, P).ndf_pdf(h["indir"])), "l")
    _add("ggx.refractSample", "ggx", "B", [V3("wt"), V1("weight"), ("refracted", 1, "b")],
         lambda c, I, P, o, m: list(_ggx(c, I, P, m).refractSample(X(I, 2), X(I, 3), out=o)),
         lambda h, P: _oggx(h, P).refract(h["x"][2], h["x"][3]), "ttf")
    for kern, ndf in (("VNDF", False), ("NDF", True)):
        _add("ggx.microfacet." + kern, "ggx", "B", [V3("m")],
             lambda c, I, P, o, m, kern=kern: _one(_ggx(c, I, P, m).microfacet(X(I, 0), X(I, 1), getattr(R, "RLS_KERNEL_" + kern),
                                                                            out=_t(o, 0))),
             lambda h, P, ndf=ndf: _one(_oggx(h, P).microfacet(h["x"][0], h["x"][1], ndf)), "t")
    _add("ggx.reflectRefract", "ggx", "B", [V3("wi"), V3("f"), V1("pdf"), V1("fresnel"), V3("wt"), V1("weight")],
         lambda c, I, P, o, m: list(_ggx(c, I, P, m).reflectRefract(X(I, 0), X(I, 1), X(I, 2), X(I, 3), out=o)),
         lambda h, P: _oggx(h, P).reflect_refract(h["x"][0], h["x"][1], h["x"][2], h["x"][3]), "tttttt")
    for lname, lobe in (("diffuse", R.RLS_RAY_DIFFUSE), ("glossy", R.RLS_RAY_GLOSSY)):
        _add(f"disney.sample.{lname}", "disney", "A", [V3("wi")],
             lambda c, I, P, o, m, lobe=lobe: _one(_disney(c, I, P, m, lobe).evalSample(X(I, 0), X(I, 1), out=_t(o, 0))),
             lambda h, P, lobe=lobe: _one(_odisney(h, P).sample(lobe, h["x"][0], h["x"][1])), "t")
        _add(f"disney.eval.{lname}", "disney", "A", [V3("f")],
             lambda c, I, P, o, m, lobe=lobe: _one(_disney(c, I, P, m, lobe).evalBrdf(I["indir"], out=_t(o, 0))),
             lambda h, P, lobe=lobe: _one(_odisney(h, P).eval(lobe, h["indir"])), "l")
        _add(f"disney.pdf.{lname}", "disney", "A", [V1("pdf")],
             lambda c, I, P, o, m, lobe=lobe: _one(_disney(c, I, P, m, lobe).evalPdf(I["indir"], out=_t(o, 0))),
             lambda h, P, lobe=lobe: _one(_odisney(h, P).pdf(lobe, h["indir"])), "l")
        _add(f"disney.sampleEvalPdf.{lname}", "disney", "A", [V3("wi"), V3("f"), V1("pdf")],
             lambda c, I, P, o, m, lobe=lobe: list(_disney(c, I, P, m, lobe).sampleEvalPdf(X(I, 0), X(I, 1), out=o)),
             lambda h, P, lobe=lobe: _odisney(h, P).sample_eval_pdf(lobe, h["x"][0], h["x"][1]), "ttt")
    for kind in (0, 1):
        _add(f"alt.sample.{kind}", "alt", "A", [V3("m")],
             lambda c, I, P, o, m, kind=kind: _one(_disney(c, I, P, m).altSample(kind, X(I, 0), X(I, 1), out=_t(o, 0))),
             lambda h, P, kind=kind: _one(_odisney(h, P).alt(kind, h["x"][0], h["x"][1])), "t")
    _add("alt.pdf", "alt", "A", [V1("pdf")], lambda c, I, P, o, m: _one(_disney(c, I, P, m).altPdf(I["indir"], out=_t(o, 0))),
         lambda h, P: _one(_odisney(h, P).alt(2, v=h["indir"])), "t")
    _add("alt.dGtr2", "alt", "A", [V1("d")], lambda c, I, P, o, m: _one(_disney(c, I, P, m).dGtr2(I["indir"], out=_t(o, 0))),
         lambda h, P: _one(_odisney(h, P).alt(3, v=h["indir"])), "t")
    _add("gauss.sample", "gauss", "A", [V1("r"), V1("pdf"), V1("profile")],
         lambda c, I, P, o, m: list(R.GaussianProfile(c, I["x"].shape[-1], P["dist_x"]).sample(X(I, 0), out=o)),
         lambda h, P: O.gauss(P["dist_x"], h["x"][0], nthreads=4), "ttt")
    _add("sss.nd_sample", "sss", "A", [V1("r"), V1("pdf"), V3("profile")],
         lambda c, I, P, o, m: list(_nd(c, I, P, m).sample(X(I, 0), out=o)), lambda h, P: _osss(h, P).nd_sample(h["x"][0]), "ttt")
    _add("sss.nd_pdf", "sss", "A", [V1("pdf")], lambda c, I, P, o, m: _one(_nd(c, I, P, m).getPdf(I["r"], out=_t(o, 0))),
         lambda h, P: _one(_osss(h, P).nd_pdf(h["r"])), "l")
    _add("sss.nd_eval", "sss", "A", [V3("profile")], lambda c, I, P, o, m: _one(_nd(c, I, P, m).evalProfile(I["r"], out=_t(o, 0))),
         lambda h, P: _one(_osss(h, P).nd_profile(h["r"])), "l")
    for nm, dpdu in (("dPdu", True), ("polar", False)):
        def run_probe(c, I, P, o, m, dpdu=dpdu):
            got = _sss(c, I, P, m, dpdu).getProbeRay(X(I, 0), X(I, 1), out=_dict_out(PROBE_KEYS, o))
            return [got[k] for k in PROBE_KEYS]

        def ref_probe(h, P, dpdu=dpdu):
            ref = _osss(h, P, dpdu).probe(h["x"][0], h["x"][1])
            return [ref[k] for k in PROBE_KEYS]
        _add("sss.probe." + nm, "sss", "A", PROBE_PLANES, run_probe, ref_probe, "tttttt")
    _add("sss.mis_pdf", "sss", "A", [V1("pdf")],
         lambda c, I, P, o, m: _one(_sss(c, I, P, m).misPdf(I["disp"], I["sN"], out=_t(o, 0))),
         lambda h, P: _one(_osss(h, P, True).mis_pdf(h["disp"], h["sN"], False)), "t")
    _add("misc.cavity_fade", "misc", "A", [V1("fade")],
         lambda c, I, P, o, m: _one(R.SssSampler.cavityFade(c, I["disp"], I["sN"], I["N"], out=_t(o, 0))),
         lambda h, P: _one(O.cavity_fade(h["disp"], h["sN"], h["N"])), "l")
    _add("misc.sample_diffuse_direction", "misc", "A", [V3("wi")],
         lambda c, I, P, o, m: _one(R.SssSampler.sampleDiffuseDirection(c, X(I, 0), X(I, 1), I["N"], I["T"], out=_t(o, 0))),
         lambda h, P: _one(O.sample_diffuse_direction(h["N"], h["T"], h["x"][0], h["x"][1])), "t")
    _add("misc.util_directions", "misc", "A", [V3("spherical"), V3("disk")],
         lambda c, I, P, o, m: list(R.util_directions(c, X(I, 0), X(I, 1), out=o)),
         lambda h, P: O.util_directions(h["x"][0], h["x"][1]), "tt")
    _add("misc.reflect_luminance", "misc", "A", [V3("reflected"), V1("luminance")],
         lambda c, I, P, o, m: list(R.util_reflect_luminance(c, I["i"], I["N"], I["col"], out=o)),
         lambda h, P: O.reflect_luminance(h["i"], h["N"], h["col"]), "bb")

    def run_skin(c, I, P, o, m):
        got = R.SkinShader(c, I["wo"], I["N"], I["T"], materials=m, **P).sampleEvalPdf(I["x"], out=_dict_out(SKIN_KEYS, o))
        return [got[k] for k in SKIN_KEYS]

    def ref_skin(h, P):
        ref = O.skin(h["wo"], h["N"], h["T"], P, h["x"], nthreads=4)
        return [ref[k] for k in SKIN_KEYS]
    _add("skin.sampleEvalPdf", "skin", "B", SKIN_PLANES, run_skin, ref_skin, "t" * len(SKIN_KEYS))
    return VERBS


def verb_names(unit=None):
    return [k for k, v in _build_verbs().items() if unit is None or v.unit == unit]


def modes(verb):
    """the per-point modes a verb has: STREAMED (every parameter a plane) and MIXED (one scalar a plain value)"""
    return ("STREAMED",) if verb.unit == "misc" else ("STREAMED", "MIXED")


def with_mode(verb, P, mode):
    return dict(P, **MIXED[verb.unit]) if mode == "MIXED" else P


def run(ctx, verb, I, P, out=None, mat=None):
    return verb.run(ctx, I, P, out, mat)


# ---- the oracle on windows ---------------------------------------------------------------------------------------------------------
def _take(v, idx, n):
    if torch.is_tensor(v):
        assert v.shape[-1] == n, (v.shape, n)
        return v[..., idx].contiguous().cpu().numpy()
    return v


def host_window(I, P, wins, n):
    """the inputs and parameters of the points of `wins` (None: all of them) on the host"""
    idx = slice(None) if wins is None else torch.cat([torch.arange(a, b, device="cuda") for a, b in wins])
    return {k: _take(v, idx, n) for k, v in I.items()}, {k: _take(v, idx, n) for k, v in P.items()}, idx


def gate(kind, got, ref, what):
    import numpy as np
    if kind == "f":
        assert int((got != ref).sum()) <= cases.flag_slack(), what
    elif kind == "b":
        cases.assert_same_bits(got, ref, what)
    elif kind == "l":
        st = cases.summarize(cases.rel_err(got, ref))
        assert st["nonfinite"] == 0 and st["max"] <= 1e-5, (what, st)
    else:
        cases.assert_tight(cases.summarize(cases.rel_err(got, np.asarray(ref))), what)


def check_windows(verb, got, I, P, wins, n, what=""):
    """the device result `got` against the oracle on the points of `wins` (None: every point), under the verb's gates"""
    hI, hP, idx = host_window(I, P, wins, n)
    ref = verb.ref(hI, hP)
    for (name, _, _), kind, g, r in zip(verb.planes, verb.gates, got, ref):
        gate(kind, g[..., idx].contiguous().cpu().numpy(), r, (verb.name, what, name))
    return ref


def bit_gates(verb):
    """the same comparison with every float plane held to the oracle's bits (the UNIFORM tests' gate under strict parity)"""
    return "".join("f" if k == "f" else "b" for k in verb.gates)


# ---- sentinel-framed output planes -------------------------------------------------------------------------------------------------
def sentinel_out(verb, n):
    """-> (buffers, views): every output plane of the verb inside a sentinel-filled buffer, PAD words (bytes) either side"""
    bufs, views = [], []
    for _, rows, kind in verb.planes:
        shape = ((rows,) if rows > 1 else ()) + (n + 2 * PAD,)
        if kind == "b":
            buf = torch.full(shape, BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
            views.append(buf[..., PAD:PAD + n])
        else:
            buf = torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")
            views.append(buf.view(torch.float32)[..., PAD:PAD + n])
        bufs.append(buf)
    return bufs, views


def check_sentinels(verb, bufs, n, what=""):
    for (name, _, kind), buf in zip(verb.planes, bufs):
        s = BYTE_SENTINEL if kind == "b" else SENTINEL
        assert bool((buf[..., :PAD] == s).all()) and bool((buf[..., PAD + n:] == s).all()), (verb.name, what, name, "padding written")
        assert not bool((buf[..., PAD:PAD + n] == s).any()), (verb.name, what, name, "a payload word was not written")


def oracle_never_yields_the_sentinel(ref):
    import numpy as np
    for r in ref:
        r = np.ascontiguousarray(r)
        if r.dtype == np.float32:
            assert not (r.view(np.uint32) == SENTINEL).any()
        else:
            assert not (r == BYTE_SENTINEL).any()


if __name__ == "__main__":
    import argparse
    import json
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-sizes", type=int, metavar="COMPUTE_UNITS", required=True)
    print(json.dumps(check_sizes(ap.parse_args().check_sizes), indent=1))
