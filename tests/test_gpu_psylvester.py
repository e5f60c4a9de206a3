"""GPU tier (MI355X): the periodic Sylvester solve and the condition of an invariant periodic subspace for ONE periodic
Schur form of any order — psd_syl_solve and psd_syl_update (csrc/psd_sylv.h) with psd_bsyl_norms and psd_bsyl_est_step —
against the dense Kronecker reference of bsylv_cases.py.  The cases are those of sylv_cases.py."""
import pytest

import bsylv_cases as sc
import psd_amd
import sylv_cases as yc
from batch_common import engine_maker

pytestmark = pytest.mark.gpu
LR = pytest.mark.parametrize("lr", ["L", "R"])
_made = {}  # the engines of this file, one per tile width


def _make():
    return psd_amd.Engine(device=0)


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
def tiled(monkeypatch, gpu_engine):
    make = engine_maker(monkeypatch, yc.KNOBS, _make, _made)
    return lambda tile: make({"PSD_SYL_TILE": str(tile)} if tile else {})


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


def test_one_tile_is_batch_kernel(tiled):
    """Within 1e-12 of the scale.  Seen on the MI355X: 0 of 34458 entries differ."""
    yc.case_one_tile(tiled(128), exact=False)


@LR
@pytest.mark.parametrize("name", ["d130a", "z130"])
def test_repeatable_bits_and_device_entry(tiled, name, lr):
    yc.case_device_equals_host(tiled(None), name, lr)


@LR
@pytest.mark.parametrize("name", ["d100", "z100"])
def test_repeatable_bits_and_device_entry_tile48(tiled, name, lr):
    yc.case_device_equals_host(tiled(48), name, lr)


@LR
@pytest.mark.parametrize("name", yc.RESID)
def test_residual_only(tiled, name, lr):
    yc.case_residual_only(tiled(None), name, lr)


@pytest.mark.parametrize("name", yc.SMALL)
def test_singular_form(tiled, name):
    yc.case_singular(tiled(4), name)


def test_arguments(tiled, make_engine):
    yc.case_arguments(tiled(None), make_engine)
