"""Array samples on the MI355X: array_samples_kernel on a device arena with
cuda destinations over the case matrix of array_sample_cases, the argument
errors (destination untouched afterwards), and CurvineArrayLoader over
HBM-tier files.  Comparisons are exact."""
import numpy as np
import pytest
import torch

from curvine_amd import native
from curvine_amd.client.filesystem import SyncFs
from curvine_amd.client.reader import SyncLocalReader
from curvine_amd.sdk import CurvineArrayLoader
from curvine_amd.testing import SyncMiniCluster
from curvine_amd.testing import test_conf as make_conf

import array_sample_cases as ac

pytestmark = pytest.mark.gpu

D = native.DTYPES
MiB = 1 << 20
CAP = 16 * MiB
DEV = "cuda:0"


@pytest.fixture(scope="module")
def arena():
    a = native.Arena(0, CAP)
    yield a
    a.close()


def tile():
    return native.load().ARRAY_TILE


@pytest.mark.parametrize("dst", ac.DSTS)
def test_exhaustive_values(arena, dst):
    ac.case_exhaustive(arena, D, DEV, dst)


@pytest.mark.parametrize("dst", ac.DSTS)
def test_residues(arena, dst):
    ac.case_residues(arena, D, DEV, dst)


@pytest.mark.parametrize("dst", ac.DSTS)
def test_splits(arena, dst):
    ac.case_splits(arena, D, DEV, dst)


@pytest.mark.parametrize("dst", ac.DSTS)
def test_long_samples(arena, dst):
    ac.case_long(arena, D, DEV, dst, tile(), CAP)


@pytest.mark.parametrize("dst", ac.DSTS)
def test_empty(arena, dst):
    ac.case_empty(arena, D, DEV, dst)


def test_rejects(arena):
    # a destination on the host side of a device arena
    host = torch.full((4096 + 512,), ac.SENTINEL, dtype=torch.uint8)
    hp = (host.data_ptr() + 4096 + 15) // 16 * 16
    extra = [("out on the host", dict(shift=hp), [])]
    ac.run_rejects(arena, D, DEV, CAP, pytest.raises, extra)
    assert bool((host == ac.SENTINEL).all())


def test_rejects_device_destination_on_host_arena():
    a = native.Arena(-1, 1 * MiB)
    try:
        img = np.random.default_rng(1).integers(0, 256, (5, 7, 3)) \
            .astype(np.uint8)
        c = ac.Call(a, D, DEV, "F32", (5, 7, 3), (3, 5), [(1, 1, 0)],
                    [1.0] * 3, [0.0] * 3)
        c.place(4096, img)
        with pytest.raises(ValueError):
            a.array_samples([(4096, 0, 0, 105)], c.rows, c.ptr, 1, c.shape,
                            c.crop, c.scale, c.bias, D["F32"], "NCHW")
        c.check()
    finally:
        a.close()


# -------------------------------------------------------------- end to end

def test_end_to_end_hbm(tmp_path, monkeypatch):
    src, labels, blobs, lblobs = ac.e2e_files()
    conf = make_conf(str(tmp_path))
    smc = SyncMiniCluster(conf=conf, tmp_dir=str(tmp_path),
                          worker_dirs=[["[HBM:512MB:0]gpu0",
                                        "[MEM:64MB]mem0"]]).start()
    made = []
    sf = None
    try:
        sf = SyncFs(smc.client_conf())
        hbm, mem, lab = [], [], []
        for i, (blob, lblob) in enumerate(zip(blobs, lblobs)):
            hbm.append(f"/arr/hbm{i}.npy")
            sf.write_file(hbm[-1], blob, storage_tier="HBM",
                          block_size=ac.E2E["block"])
            mem.append(f"/arr/mem{i}.npy")
            sf.write_file(mem[-1], blob, storage_tier="MEM",
                          block_size=ac.E2E["block"])
            lab.append(f"/arr/lab{i}.npy")
            sf.write_file(lab[-1], lblob, storage_tier="MEM")

        calls, slows = [], []
        orig = native.Arena.array_samples
        orig_exec = SyncLocalReader.exec_array_samples

        def spy(self, pieces, *a, **kw):
            calls.append((self.device, list(pieces)))
            return orig(self, pieces, *a, **kw)

        def spy_exec(self, groups, slow, *a, **kw):
            slows.append((list(groups), list(slow)))
            return orig_exec(self, groups, slow, *a, **kw)
        monkeypatch.setattr(native.Arena, "array_samples", spy)
        monkeypatch.setattr(SyncLocalReader, "exec_array_samples", spy_exec)

        def maker(paths):
            def make(**kw):
                kw.setdefault("labels", lab)
                ld = CurvineArrayLoader(smc.client_conf(), paths,
                                        ac.E2E["batch"], device=DEV, **kw)
                made.append(ld)
                return ld
            return make

        ac.check_loader(maker(hbm), src, labels)
        # the device arena took pieces that begin inside a sample, and
        # nothing went the slow way
        assert calls and all(d == 0 for d, _ in calls)
        assert any(p[2] > 0 for _, ps in calls for p in ps)
        assert slows and not any(s for _g, s in slows)

        # MEM-tier files with cuda destinations: every sample the slow way,
        # the same tensors
        del calls[:], slows[:]
        ac.check_loader(maker(mem), src, labels)
        assert not calls and slows
        assert all(not g for g, _s in slows)
        assert sum(len(s) for _g, s in slows) > len(src)
    finally:
        for ld in made:
            ld.close()
        if sf is not None:
            sf.shutdown()
        smc.stop()
