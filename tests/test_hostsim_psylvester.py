"""CPU tier: the periodic Sylvester solve and the condition of an invariant periodic subspace for ONE periodic Schur form
of any order (Engine.psylvester, Engine.subspacecond; csrc/psd_sylv.h) on the TEST-ONLY serial simulation of the device
code, against the dense Kronecker reference of bsylv_cases.py.  The cases are those of sylv_cases.py."""
import os

import pytest

import bsylv_cases as sc
import psd_amd
import sylv_cases as yc
from batch_common import engine_maker

_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim", "_build", "libpsd_hostsim.so")
LR = pytest.mark.parametrize("lr", ["L", "R"])
_made = {}  # the engines of this file, one per tile width


def _make():
    return psd_amd.Engine(libpath=_LIB)


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _made.values():
        e.close()
    _made.clear()


@pytest.fixture
def make_engine(monkeypatch):
    return engine_maker(monkeypatch, yc.KNOBS, _make, {})


@pytest.fixture
def tiled(monkeypatch):
    make = engine_maker(monkeypatch, yc.KNOBS, _make, _made)
    return lambda tile: make({"PSD_SYL_TILE": str(tile)} if tile else {})


@LR
@pytest.mark.parametrize("name", yc.SMALL + yc.BIG + yc.WIDE)
def test_reference_inputs(name, lr):
    yc.case_reference_inputs(name, lr)


@LR
@pytest.mark.parametrize("tile", [4, 2, 5])
@pytest.mark.parametrize("name", yc.SMALL)
def test_small_tiles(tiled, name, lr, tile):
    yc.case_small_tiles(tiled(tile), name, lr, tile)


@LR
@pytest.mark.parametrize("k", range(len(sc.PROBLEMS)), ids=sc.IDS)
def test_batch_problems_tile4(tiled, k, lr):
    yc.case_batch_problems(tiled(4), k, lr)


@LR
@pytest.mark.parametrize("name,tile", [(name, t) for name in yc.WIDE for t in yc.WIDE_TILES[name]])
def test_wide_tiles(tiled, name, lr, tile):
    yc.case_wide_tiles(tiled(tile), name, lr, tile)


@LR
@pytest.mark.parametrize("tile", yc.WIDE_BATCH_TILES)
@pytest.mark.parametrize("k", yc.WIDE_BATCH, ids=[sc.IDS[k] for k in yc.WIDE_BATCH])
def test_wide_tiles_batch_problems(tiled, k, lr, tile):
    yc.case_wide_tiles(tiled(tile), k, lr, tile)


@LR
@pytest.mark.parametrize("name", yc.BIG)
def test_above_batch_cap(tiled, name, lr):
    yc.case_above_cap(tiled(None), name, lr)


def test_one_tile_is_batch_kernel_bits(tiled):
    yc.case_one_tile(tiled(128), exact=True)


@LR
@pytest.mark.parametrize("name", ["d130a", "z130"])
def test_repeatable_bits(tiled, name, lr):
    yc.case_repeat(tiled(None), name, lr)


@LR
@pytest.mark.parametrize("name", ["d100", "z100"])
def test_repeatable_bits_tile48(tiled, name, lr):
    yc.case_repeat(tiled(48), name, lr)


@pytest.mark.parametrize("name", yc.SMALL)
def test_singular_form(tiled, name):
    yc.case_singular(tiled(4), name)


def test_arguments(tiled, make_engine):
    yc.case_arguments(tiled(None), make_engine)
