"""Token windows on the MI355X: token_windows_kernel on a device arena
with cuda destinations over the case matrix of token_window_cases, the
argument errors (destinations untouched afterwards), and
CurvineTokenLoader over HBM-tier files.  Comparisons are exact."""
import numpy as np
import pytest
import torch

from curvine_amd import errors as err
from curvine_amd import native
from curvine_amd.client.filesystem import SyncFs
from curvine_amd.client.reader import SyncLocalReader
from curvine_amd.sdk import CurvineTokenLoader
from curvine_amd.testing import SyncMiniCluster
from curvine_amd.testing import test_conf as make_conf

import token_window_cases as tc

pytestmark = pytest.mark.gpu

D = native.DTYPES
MiB = 1 << 20
CAP = 16 * MiB
DEV = "cuda:0"
BLOCK = 64


@pytest.fixture(scope="module")
def arena():
    a = native.Arena(0, CAP)
    yield a
    a.close()


def tile():
    return native.load().TOKEN_TILE


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_residues(arena, src, dst):
    tc.case_residues(arena, D, DEV, src, dst)


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_splits(arena, src, dst):
    tc.case_splits(arena, D, DEV, src, dst)


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_long_window(arena, src, dst):
    tc.case_long(arena, D, DEV, src, dst, tile())


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_vocab_count(arena, src, dst):
    tc.case_vocab(arena, D, DEV, src, dst, tile())


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_empty(arena, src, dst):
    tc.case_empty(arena, D, DEV, src, dst)


def test_rejects(arena):
    # a destination on the host side of a device arena
    host = torch.full((4096 + 512,), tc.SENTINEL, dtype=torch.uint8)
    hp = (host.data_ptr() + 4096 + 15) // 16 * 16
    ok = (4096, 0, 0, 9)
    extra = [("x on the host", [ok], hp, 0, tc.ROWS, 8, D["U16"], D["I64"]),
             ("y on the host", [ok], 0, hp, tc.ROWS, 8, D["U16"], D["I64"])]
    tc.run_rejects(arena, D, DEV, CAP, pytest.raises, extra)
    assert bool((host == tc.SENTINEL).all())


def test_rejects_device_destination_on_host_arena():
    a = native.Arena(-1, 1 * MiB)
    try:
        c = tc.Call(a, D, DEV, "U16", "I64", 8)
        c.place(4096, tc.make_tokens(np.random.default_rng(1), "U16", 9))
        with pytest.raises(ValueError):
            a.token_windows([(4096, 0, 0, 9)], c.x_ptr, c.y_ptr, tc.ROWS, 8,
                            D["U16"], D["I64"], 0)
        c.check()
    finally:
        a.close()


# -------------------------------------------------------------- end to end

def test_end_to_end_hbm(tmp_path, monkeypatch):
    files = tc.e2e_files()
    ref = tc.e2e_reference(files)
    conf = make_conf(str(tmp_path))
    smc = SyncMiniCluster(conf=conf, tmp_dir=str(tmp_path),
                          worker_dirs=[["[HBM:512MB:0]gpu0",
                                        "[MEM:64MB]mem0"]]).start()
    made = []
    sf = None
    try:
        sf = SyncFs(smc.client_conf())
        hbm, mem = [], []
        for i, blob in enumerate(files):
            hbm.append(f"/tok/hbm{i}.bin")
            sf.write_file(hbm[-1], blob, storage_tier="HBM", block_size=BLOCK)
            mem.append(f"/tok/mem{i}.bin")
            sf.write_file(mem[-1], blob, storage_tier="MEM", block_size=BLOCK)
        sf.write_file("/tok/five.bin", b"12345", storage_tier="HBM")

        calls, slows = [], []
        orig = native.Arena.token_windows
        orig_exec = SyncLocalReader.exec_token_windows

        def spy(self, pieces, *a, **kw):
            calls.append((self.device, list(pieces)))
            return orig(self, pieces, *a, **kw)

        def spy_exec(self, groups, slow, *a, **kw):
            slows.append(list(slow))
            return orig_exec(self, groups, slow, *a, **kw)
        monkeypatch.setattr(native.Arena, "token_windows", spy)
        monkeypatch.setattr(SyncLocalReader, "exec_token_windows", spy_exec)

        def maker(paths):
            def make(**kw):
                ld = CurvineTokenLoader(smc.client_conf(), paths, tc.E2E["T"],
                                        tc.E2E["batch"], device=DEV,
                                        src_dtype=tc.E2E["src"],
                                        header_bytes=tc.E2E["header"], **kw)
                made.append(ld)
                return ld
            return make

        tc.check_loader(maker(hbm), ref,
                        lambda: pytest.raises(err.InvalidArgument))
        # the device arena took pieces that begin inside a window, and the
        # tokens cut by a block boundary went the slow way, one at a time
        assert calls and all(d == 0 for d, _ in calls)
        assert any(p[2] > 0 for _, ps in calls for p in ps)
        assert any(s for s in slows)
        assert all(n == 1 for s in slows for _o, _r, _j, n in s)

        ld = maker(hbm)(out_dtype=torch.int32)
        x, y = next(iter(ld))
        assert x.is_cuda and y.is_cuda and x.dtype == torch.int32
        tc.check_order(ld, tc.e2e_reference(files, "I32"),
                       list(range(ld.num_windows)))

        # MEM-tier files with cuda destinations: everything the slow way,
        # the same tensors
        del calls[:], slows[:]
        ld = maker(mem)(drop_last=False)
        tc.check_order(ld, ref, list(range(len(ref[0]))), drop_last=False)
        assert not calls and slows and all(slows)

        with pytest.raises(err.InvalidArgument):
            CurvineTokenLoader(smc.client_conf(), ["/tok/five.bin"], 2, 1,
                               device=DEV)
    finally:
        for ld in made:
            ld.close()
        if sf is not None:
            sf.shutdown()
        smc.stop()
