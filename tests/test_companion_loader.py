"""CPU: the one loader of the companion libraries (rlshaders_amd/_capi.py, load_companion) and the one set of tensor checks the
probe walk, the shadow walk and the nearest-hit wrappers share (rlshaders_amd/walk.py, _rows and _flat).

The loader: through every module's environment override a path that does not exist refuses by the module's name with the build
function that makes the library.  A module loads once and keeps the library, so the test empties its ``_lib`` to load again.

The checks: no device is needed to take the shape and stride branch of ``_rows`` -- a CPU tensor is refused first, as ever, so
the planes here are CPU tensors of a subclass that answers ``is_cuda`` with True.  Their addresses go into a struct and no
further: nothing is called with them."""
import pytest
import torch

MODULES = {"trace": "RLSHADERS_AMD_TRACE_LIB", "walk": "RLSHADERS_AMD_WALK_LIB", "shadow_walk": "RLSHADERS_AMD_SHADOW_WALK_LIB",
           "nearest": "RLSHADERS_AMD_NEAREST_LIB", "nearest_refit": "RLSHADERS_AMD_NEAREST_REFIT_LIB"}


@pytest.fixture(scope="module")
def built():
    from rlshaders_amd import build
    for name in MODULES:
        getattr(build, f"build_{name}_library")()


@pytest.mark.parametrize("name", sorted(MODULES))
def test_a_missing_library_is_refused_by_module_and_build_function(built, monkeypatch, tmp_path, name):
    import importlib
    module = importlib.import_module(f"rlshaders_amd.{name}")
    lib = module.load()                                             # from its own place
    absent = tmp_path / f"absent_{name}.so"
    monkeypatch.setenv(MODULES[name], str(absent))
    assert module.load() is lib                                     # loaded once: the module keeps it
    monkeypatch.setattr(module, "_lib", None)
    with pytest.raises(RuntimeError) as e:
        module.load()
    assert str(e.value) == (f"rlshaders_amd.{name}: {absent} not found. Build it with "
                            f"`python -c 'from rlshaders_amd import build; build.build_{name}_library()'` (needs hipcc).")
    assert module._lib is None


def test_a_library_without_the_symbols_is_refused(built, monkeypatch):
    from rlshaders_amd import build, walk
    monkeypatch.setenv("RLSHADERS_AMD_WALK_LIB", str(build.TRACE_LIB))
    monkeypatch.setattr(walk, "_lib", None)
    with pytest.raises(RuntimeError) as e:
        walk.load()
    assert str(e.value) == f"rlshaders_amd.walk: {build.TRACE_LIB} lacks C-ABI symbols: {list(walk.PROTOTYPES)}"


class OnDevice(torch.Tensor):
    """a CPU tensor that says it is on the device"""
    is_cuda = property(lambda self: True)


def dev(t: torch.Tensor) -> torch.Tensor:
    return t.as_subclass(OnDevice)


def planes(width: int, step: int = 1) -> torch.Tensor:
    """float32 [3, width], a view with inner stride `step`"""
    t = dev(torch.zeros(3, width * step))[:, ::step]
    assert t.is_cuda and tuple(t.shape) == (3, width) and (width == 1 or t.stride(1) == step)
    return t


def users(P, n):
    """the three wrappers' struct builders over the planes P, n entries"""
    from rlshaders_amd import nearest, shadow_walk, walk
    hit, t = dev(torch.zeros(n, dtype=torch.uint8)), dev(torch.zeros(n))
    return {"walk": lambda: walk.Found(hit, t, P, P, P).struct(n),
            "shadow_walk": lambda: shadow_walk.Found(hit, t, P, P).struct(n),
            "nearest": lambda: nearest.Rays(P, P, rays=n).struct()}


def test_one_element_planes_of_any_stride_are_accepted_by_all_three():
    P = planes(1, step=2)
    assert P.stride(1) == 2
    for name, struct in users(P, 1).items():
        s = struct()
        first = s.P if name != "nearest" else s.origin
        assert (first.x, first.y, first.z) == tuple(P[k].data_ptr() for k in range(3)), name


def test_wider_planes_need_unit_inner_stride_and_a_device():
    for name, struct in users(planes(2), 2).items():
        struct()                                                             # unit stride: accepted
    for name, struct in users(planes(2, step=2), 2).items():
        with pytest.raises(ValueError, match=r"expected a float32 CUDA tensor \[3, >= 2\] with unit inner stride"):
            struct()
    cpu = torch.zeros(3, 1)
    for name, struct in users(cpu, 1).items():
        with pytest.raises(ValueError, match="expected a"):                  # a CPU tensor is refused as before
            struct()


def test_the_checks_are_written_once():
    from rlshaders_amd import nearest, shadow_walk, walk
    assert shadow_walk._rows is walk._rows is nearest._rows and shadow_walk._flat is walk._flat is nearest._flat
