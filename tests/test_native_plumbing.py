"""The shared plumbing of the native kernel entry points (scratch carver,
tile tables, per-device CRC tables), on a host arena and, marked gpu, on
device 0.  The case bodies are in native_plumbing_cases.py."""
import pytest

import kernel_edge_cases as edges
import native_plumbing_cases as cases
from curvine_amd import native


def test_scratch_reuse_host():
    a = native.Arena(-1, 8 << 20)
    try:
        cases.scratch_reuse(a, edges.HostDst)
    finally:
        a.close()


def test_crc_two_arenas_host():
    cases.crc_two_arenas(-1)


@pytest.mark.gpu
def test_scratch_reuse_device():
    assert native.gpu_available(), "GPU required: _native must see a device"
    a = native.Arena(0, 8 << 20, staging_bytes=1 << 20, staging_count=2)
    try:
        cases.scratch_reuse(a, edges.TorchDst)
    finally:
        a.close()


@pytest.mark.gpu
def test_crc_two_arenas_device():
    assert native.gpu_available(), "GPU required: _native must see a device"
    cases.crc_two_arenas(0)
