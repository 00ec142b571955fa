"""GPU tests (MI355X): the compressor edge cases of lz4_compress_cases.py on
a device arena, i.e. through lz4_compress_kernel, with
lz4_decompress_kernel as one of the three decoders.
test_lz4_compress_cases.py runs the same bodies on a host arena.

What each test reaches in the kernel that whole-buffer kinds meet only by
chance:

  test_planted[literal]    lz4c_emit_ext on a literal field of 14/15/16 and
                           15 + 255k, lz4c_emit_lits either side of 256
  test_planted[match*]     the match field at 18/19/20 and 19 + 255k, the
                           256-byte passes of the extension loop at 4 + 256k,
                           candidates from the position table (offset 100)
                           and from the in-step table (offset 37)
  test_planted[period]     overlapping matches at every offset 1..70, from
                           both tables
  test_length_coverage     the lengths above were emitted, not skipped by
                           late starts
  test_store_alignment     the uint4 literal stores at every residue
  test_source_residue      the head/body/tail staging split at every g & 15
  test_chunk_independence  no state carried from chunk to chunk or call to
                           call
  test_*_chunk_ends        mflimit and mend
  test_largest_call        256 chunks, every one decoded
"""
import json

import pytest

import lz4_compress_cases as cases
from curvine_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert native.gpu_available(), "GPU required: _native must see a device"
    a = native.Arena(0, cases.ARENA_BYTES, staging_bytes=4 << 20,
                     staging_count=4)
    yield cases.Ctx(a, native, 1 << 20)
    a.close()


@pytest.mark.parametrize("family", cases.PLANTED_FAMILIES)
def test_planted(ctx, family):
    cases.planted_family(ctx, family)


def test_length_coverage(ctx):
    cases.coverage(ctx)


def test_recorded_figures(ctx):
    """Recorded, not asserted: profiles/lz4_compress_edges.json keeps this
    line for the kernel."""
    print("lz4_compress_edges device " + json.dumps(cases.recorded(ctx)))


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
