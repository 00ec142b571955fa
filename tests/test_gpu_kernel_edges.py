"""GPU tests (MI355X): the edge matrices of kernel_edge_cases.py on a device
arena, i.e. through crc32c_kernel, copy_extents_kernel, fill_kernel and
lz4_decompress_kernel.  test_kernel_refs.py runs the same bodies on a host
arena, so the expectations are checked where no device is involved.

Every comparison is bitwise.  What each test reaches that the cases in
test_gpu.py do not:

  test_crc_matrix        the ragged branch of the in-kernel tree combine
                         (right_n < stride) at every level, the host-side
                         combine of a partial last workgroup, offsets that
                         are not a multiple of 8
  test_crc_coverage      every sub-chunk of a ragged count enters the CRC
  test_gather_tile_paths the 16-byte, 4-byte and byte paths across tile
                         boundaries
  test_gather_alignment  each path choice by source, destination and length
  test_gather_grid_stride, test_fill_grid_stride, chunks_16_x16400
                         the three grid-stride loops
  test_gather_empty, lz4 "empty"
                         calls that used to launch a grid of 0
  test_fill_matrix       uint4 stores at every residue of the destination
  test_lz4_malformed     the error flag for every container the host
                         decoder rejects, a short decode included
"""
import pytest

import kernel_edge_cases as edges
from curvine_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arena():
    assert native.gpu_available(), "GPU required: _native must see a device"
    a = native.Arena(0, 64 << 20, staging_bytes=4 << 20, staging_count=4)
    yield a
    a.close()


@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
def test_crc_matrix(arena, kind):
    edges.crc_matrix(arena, kind)


def test_crc_small(arena):
    edges.crc_small(arena)


def test_crc_coverage(arena):
    edges.crc_coverage(arena)


@pytest.mark.parametrize("path", edges.TILE_PATHS)
def test_gather_tile_paths(arena, path):
    edges.gather_tile_paths(arena, edges.TorchDst, path)


def test_gather_alignment(arena):
    edges.gather_alignment(arena, edges.TorchDst)


def test_gather_grid_stride(arena):
    edges.gather_grid_stride(arena, edges.TorchDst)


def test_gather_empty(arena):
    edges.gather_empty(arena, edges.TorchDst)


@pytest.mark.parametrize("residue", range(16))
def test_fill_matrix(arena, residue):
    """fill_kernel casts its destination to uint4* at whatever alignment the
    offset has.  Offsets of every residue mod 16, with guard bytes either
    side, are pinned here against a numpy model."""
    edges.fill_matrix(arena, residue)


def test_fill_grid_stride(arena):
    edges.fill_grid_stride(arena)


@pytest.mark.parametrize("name", edges.WELL_FORMED)
def test_lz4_well_formed(arena, name):
    edges.lz4_decode(arena, name)


@pytest.mark.parametrize("name", edges.MALFORMED)
def test_lz4_malformed(arena, name):
    edges.lz4_reject(arena, name)
