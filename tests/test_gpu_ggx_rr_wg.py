"""GPU: ggx_rr_wg_kernel (rlshaders_amd/csrc_rr/) -- BASELINE config 2's kernel with one uniform-slope pass per workgroup tile --
against the frozen ggx_kernel<5, 0, 1> it stands in for, both driven through rls_ggx_reflect_refract: this process launches the
companion's kernel, a process started with RLS_GGX_RR_WG=0 (the switch is read once per process) the frozen one, once for
every case (tests/rr_wg_util.py).

The gate: 0 differing words on all twelve output planes, NaN equal to NaN by bit pattern, no point excluded; and against the
oracle the gates of tests/cases.py (bit equality where the host libm is the build the device libm follows).

  sizes      n = 1 .. 2^16 + 77 on cases.ggx_mixed: partial tiles only, a partial tile behind full ones, grids that are and are
             not a multiple of 8 (n = 257: two workgroups, plain mapping; n = 8 * 256 + 1: sixteen workgroups on per-XCD
             eighths of two tiles each, of which eight walk one full tile, one the one-point tile and seven none);
  requests   0, 1, 64, 66 and 512 requests in one tile, all in the first or in the last wavefront, and the same patterns
             across two tiles; rx = 0 on one sample only;
  rounds     a capped grid walks the batch in two and a half rounds, tiles without a request between tiles with some;
  hostile    NaN, infinities and values outside [0, 1) in xi and roughness; untouched points keep the clean run's bits;
  sentinel   nothing but the n words of each plane is written."""
import numpy as np
import pytest
import torch

import cases
import rlshaders_amd as R
import rr_wg_util as U
from gpu_util import ggx_oracle

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD            # a quiet NaN with a payload: no kernel writes it


@pytest.fixture(scope="module")
def frozen(gpu, tmp_path_factory):
    """the frozen arm of every case, from one process of its own"""
    from rlshaders_amd import build
    assert build.RR_LIB.exists(), "librls_ggx_rr.so is not built: this process would run the frozen kernel too"
    return U.frozen_results(tmp_path_factory.mktemp("rr_wg_frozen"))


def _parity(gpu, frozen, name, oracle=None):
    c, x = U.case(name)
    got = U.run(gpu, c, x)
    assert U.companion_loaded(), "this process ran the frozen kernel: the companion was not found or is switched off"
    d = U.differing_words(got, frozen[name])
    print(name, "n", x.shape[1], "words differing from the frozen kernel:", d, "requests per tile:",
          U.per_tile_requests(c, x)[:4])
    assert d == 0, (name, d)
    if oracle is not None:
        ref = ggx_oracle(oracle, c).reflect_refract(x[0], x[1], x[2], x[3])
        for nm, a, b in zip(U.NAMES, got, ref):
            cases.assert_tight(cases.summarize(cases.rel_err(a, b)), f"{name} {nm}")
    return got


@pytest.mark.parametrize("n", U.SIZES)
def test_sizes_against_the_frozen_kernel_and_the_oracle(gpu, oracle, frozen, n):
    _parity(gpu, frozen, f"mixed:{n}", oracle)


@pytest.mark.parametrize("layout", sorted(U.LAYOUTS))
@pytest.mark.parametrize("name", sorted(U.RECIPES))
def test_request_count_edges(gpu, oracle, frozen, name, layout):
    _parity(gpu, frozen, f"recipe:{name}@{layout}", oracle)


@pytest.mark.parametrize("sample", [0, 1])
def test_rx_zero_on_one_sample_only(gpu, oracle, frozen, sample):
    c, x = U.case(f"rx0:{sample}")
    n1, n2, _, _ = U.requests(c, x)
    assert (n1 != n2).sum() == len(range(0, x.shape[1], 3)) and (n2 if sample else n1).sum() == (n1 | n2).sum()
    _parity(gpu, frozen, f"rx0:{sample}", oracle)


def test_tiles_reuse_the_queue_round_after_round(frozen):
    """two and a half rounds of the tile loop (a context capped at one workgroup per CU), tiles with and without requests"""
    mp = pytest.MonkeyPatch()
    mp.setenv("RLS_BLOCKS_PER_CU", "1")
    try:
        ctx = R.Context(0)
    finally:
        mp.undo()
    try:
        c, x = U.case("rounds:")
        got = U.run(ctx, c, x)
    finally:
        ctx.close()
    d = U.differing_words(got, frozen["rounds:"])
    assert d == 0, d


def test_hostile_inputs(gpu, frozen):
    c, x, touched = U.hostile(True)
    got = U.run(gpu, c, x)
    assert sum(int(np.isnan(a).sum()) for a in got) > 0                       # the poison reaches the outputs
    assert U.differing_words(got, frozen["hostile:poisoned"]) == 0
    n1, n2, _, _ = U.requests(*U.hostile(False)[:2])
    req = n1 | n2
    assert (touched & req).sum() > 20 and (touched & ~req).sum() > 20        # over requesting and quiet lanes alike
    clean = U.run(gpu, *U.hostile(False)[:2])
    keep = ~touched
    assert keep.sum() > x.shape[1] // 2
    assert U.differing_words([a[..., keep] for a in got], [a[..., keep] for a in clean]) == 0


@pytest.mark.parametrize("n", [513, 255])
def test_output_planes_leave_the_words_beside_them(gpu, frozen, n):
    pad = 67
    c, x = U.case(f"mixed:{n}")
    bufs = []

    def alloc(*rows):
        buf = torch.full(rows + (n + 2 * pad,), SENTINEL, dtype=torch.int32, device="cuda")
        bufs.append(buf)
        return buf.view(torch.float32)[..., pad:pad + n]

    out = (alloc(3), alloc(3), alloc(), alloc(), alloc(3), alloc())
    got = U.run(gpu, c, x, out=out)
    assert U.differing_words(got, frozen[f"mixed:{n}"]) == 0
    for buf in bufs:
        h = buf.cpu().numpy()
        assert (h[..., :pad] == SENTINEL).all() and (h[..., pad + n:] == SENTINEL).all()
