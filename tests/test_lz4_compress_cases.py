"""The compressor edge cases of lz4_compress_cases.py on a host arena, i.e.
through lz4_compress_block and the host decoders.
test_gpu_lz4_compress_edges.py runs the same bodies on a device arena."""
import json

import pytest

import lz4_compress_cases as cases
from curvine_amd import native


@pytest.fixture(scope="module")
def ctx():
    a = native.Arena(-1, cases.ARENA_BYTES)
    yield cases.Ctx(a, native, 1 << 20)
    a.close()


@pytest.mark.parametrize("family", cases.PLANTED_FAMILIES)
def test_planted(ctx, family):
    cases.planted_family(ctx, family)


def test_length_coverage(ctx):
    cases.coverage(ctx)


def test_recorded_figures(ctx):
    """Recorded, not asserted: profiles/lz4_compress_edges.json keeps this
    line for the host codec."""
    print("lz4_compress_edges host " + json.dumps(cases.recorded(ctx)))


def test_store_alignment(ctx):
    cases.store_alignment(ctx)


def test_source_residue(ctx):
    cases.source_residue(ctx)


def test_chunk_independence(ctx):
    cases.chunk_independence(ctx)


def test_small_chunk_ends(ctx):
    cases.small_chunk_ends(ctx)


@pytest.mark.parametrize("kind", cases.END_KINDS)
def test_full_chunk_ends(ctx, kind):
    cases.full_chunk_ends(ctx, kind)


@pytest.mark.parametrize("n", [16 << 20, (16 << 20) - 65535])
def test_largest_call(ctx, n):
    cases.largest_call(ctx, n)
