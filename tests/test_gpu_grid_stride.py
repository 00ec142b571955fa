"""The grid-stride cases on the MI355X: every tiled typed, token and array
kernel launched with min(n_tiles, TILE_GRID_CAP) workgroups for at least
2 * TILE_GRID_CAP + 300 tiles, so every workgroup runs two or three
different tiles.  The cases, their references and what each of them pins
are in tests/grid_stride_cases.py; tests/test_grid_stride.py runs the same
cases on a host arena."""
import pytest

from curvine_amd import native

import grid_stride_cases as gs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tier():
    a = native.Arena(0, gs.ARENA_BYTES)
    yield gs.Tier(native, a, 0)
    a.close()


def test_convert_plain(tier):
    gs.case_cast(tier, store=False)


def test_store_plain(tier):
    gs.case_cast(tier, store=True)


@pytest.mark.parametrize("store", [True, False], ids=["store", "load"])
def test_scaled(tier, store):
    gs.case_cast(tier, store=store, scaled=True)


@pytest.mark.parametrize("src,dst", gs.TOKEN_PAIRS)
def test_token_windows(tier, src, dst):
    gs.case_token_windows(tier, src, dst)


def test_absmax(tier):
    gs.case_absmax(tier)


@pytest.mark.parametrize("dst,layout", gs.ARRAY_COMBOS)
def test_array_samples(tier, dst, layout):
    gs.case_array_samples(tier, dst, layout)


@pytest.mark.parametrize("src", ["U16", "I32"])
def test_token_eos_index(tier, src):
    gs.case_token_eos(tier, src)


@pytest.mark.parametrize("src,dst", gs.PACK_PAIRS)
def test_token_pack(tier, src, dst):
    gs.case_token_pack(tier, src, dst)


def test_token_pack_cu_loop(tier):
    gs.case_token_pack_cu(tier, "U16", "I32")


def test_block_absmax(tier):
    gs.case_block_absmax(tier)


@pytest.mark.parametrize("mode", gs.MX_MODES)
def test_mx(tier, mode):
    gs.case_mx(tier, mode)


@pytest.mark.parametrize("store", [True, False], ids=["store", "load"])
def test_block_scaled(tier, store):
    gs.case_cast(tier, store=store, block=True)
