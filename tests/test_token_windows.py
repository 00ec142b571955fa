"""Token windows without a GPU: the host twin of token_windows_kernel on a
host arena, the argument errors, and CurvineTokenLoader over MEM-tier files
with device="cpu".  Expected values come from token_window_cases (numpy
only); comparisons are exact."""
import numpy as np
import pytest

from curvine_amd import errors as err
from curvine_amd import native
from curvine_amd.client.filesystem import SyncFs
from curvine_amd.client.reader import SyncLocalReader
from curvine_amd.sdk import CurvineTokenLoader
from curvine_amd.testing import SyncMiniCluster
from curvine_amd.testing import test_conf as make_conf

import token_window_cases as tc

D = native.DTYPES
MiB = 1 << 20
CAP = 4 * MiB
BLOCK = 64


@pytest.fixture(scope="module")
def arena():
    a = native.Arena(-1, CAP)
    yield a
    a.close()


def tile():
    return native.load().TOKEN_TILE


def test_names():
    assert native.TOKEN_SOURCES == ("U16", "U32", "I32")
    assert native.TOKEN_TARGETS == ("I32", "I64")
    ok = {(s, d) for s in D for d in D if native.token_windows_supported(s, d)}
    assert ok == set(tc.PAIRS)
    assert tile() >= 64


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_residues(arena, src, dst):
    tc.case_residues(arena, D, "cpu", src, dst)


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_splits(arena, src, dst):
    tc.case_splits(arena, D, "cpu", src, dst)


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_long_window(arena, src, dst):
    tc.case_long(arena, D, "cpu", src, dst, tile())


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_vocab_count(arena, src, dst):
    tc.case_vocab(arena, D, "cpu", src, dst, tile())


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_empty(arena, src, dst):
    tc.case_empty(arena, D, "cpu", src, dst)


def test_rejects(arena):
    tc.run_rejects(arena, D, "cpu", CAP, pytest.raises)


@pytest.mark.parametrize("src,dst", tc.PAIRS)
def test_token_convert_host(src, dst):
    rng = np.random.default_rng(3)
    t = tc.make_tokens(rng, src, 41)
    for shift in (0, 1):                    # an odd source address too
        raw = bytearray(shift) + bytearray(t.tobytes())
        out = native.token_convert_host(memoryview(raw)[shift:], D[src],
                                        D[dst], len(t))
        assert out == tc.ref_widen(t, dst).tobytes()
    assert native.token_convert_host(b"", D[src], D[dst], 0) == b""
    with pytest.raises(ValueError):
        native.token_convert_host(t.tobytes(), D[src], D[dst], len(t) + 1)
    with pytest.raises(ValueError):
        native.token_convert_host(t.tobytes(), D["U32"], D["I32"], 1)


# -------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def cluster(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("tokens"))
    smc = SyncMiniCluster(conf=make_conf(tmp), tmp_dir=tmp).start()
    sf = SyncFs(smc.client_conf())
    files = tc.e2e_files()
    paths = []
    for i, blob in enumerate(files):
        paths.append(f"/tok/f{i}.bin")
        sf.write_file(paths[-1], blob, storage_tier="MEM", block_size=BLOCK)
    sf.write_file("/tok/five.bin", b"12345", storage_tier="MEM")
    yield smc, files, paths
    sf.shutdown()
    smc.stop()


def test_end_to_end_mem(cluster, monkeypatch):
    smc, files, paths = cluster
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

    made = []

    def make(**kw):
        ld = CurvineTokenLoader(smc.client_conf(), paths, tc.E2E["T"],
                                tc.E2E["batch"], device="cpu",
                                src_dtype=tc.E2E["src"],
                                header_bytes=tc.E2E["header"], **kw)
        made.append(ld)
        return ld
    try:
        tc.check_loader(make, tc.e2e_reference(files),
                        lambda: pytest.raises(err.InvalidArgument))
        # the host arena took pieces that begin inside a window, and the
        # tokens cut by a block boundary went the slow way, one at a time
        assert calls and all(d == -1 for d, _ in calls)
        assert any(p[2] > 0 for _, ps in calls for p in ps)
        assert any(s for s in slows)
        assert all(n == 1 for s in slows for _o, _r, _j, n in s)

        import torch
        ld = make(out_dtype=torch.int32)
        tc.check_order(ld, tc.e2e_reference(files, "I32"),
                       list(range(ld.num_windows)))
    finally:
        for ld in made:
            ld.close()


def test_loader_argument_errors(cluster):
    import torch
    smc, _files, paths = cluster
    conf = smc.client_conf()
    with pytest.raises(err.InvalidArgument):
        CurvineTokenLoader(conf, ["/tok/five.bin"], 2, 1, device="cpu")
    with pytest.raises(err.InvalidArgument):      # shorter than its header
        CurvineTokenLoader(conf, ["/tok/five.bin"], 2, 1, device="cpu",
                           header_bytes=7)
    for kw in (dict(src_dtype="U32", out_dtype=torch.int32),
               dict(src_dtype="U8"), dict(out_dtype=torch.int16),
               dict(src_dtype="F32")):
        with pytest.raises(err.Unsupported):
            CurvineTokenLoader(conf, paths, 8, 2, device="cpu", **kw)
    for kw in (dict(seq_len=0), dict(seq_len=-1), dict(batch_size=0),
               dict(stride=0), dict(stride=-3), dict(rank=2, world=2),
               dict(rank=-1), dict(world=0), dict(header_bytes=-1)):
        args = dict(seq_len=8, batch_size=2)
        args.update(kw)
        with pytest.raises(err.InvalidArgument):
            CurvineTokenLoader(conf, paths, device="cpu", **args)


def test_windows_stride_and_short_file(cluster):
    smc, files, paths = cluster
    conf = smc.client_conf()
    T, hdr = 20, tc.E2E["header"]
    ld = CurvineTokenLoader(conf, paths, T, 5, device="cpu", header_bytes=hdr,
                            stride=7, drop_last=False)
    try:
        xs, ys = tc.collect(ld)
        ref = [tc.ref_file_windows(b, "U16", "I64", hdr, T, 7) for b in files]
        assert np.array_equal(np.concatenate(xs),
                              np.concatenate([r[0] for r in ref]))
        assert np.array_equal(np.concatenate(ys),
                              np.concatenate([r[1] for r in ref]))
    finally:
        ld.close()
    # a file with fewer than seq_len + 1 tokens has no windows
    ld = CurvineTokenLoader(conf, ["/tok/five.bin"], 2, 1, device="cpu",
                            header_bytes=1)
    try:
        assert ld.num_windows == 0 and len(ld) == 0 and list(ld) == []
    finally:
        ld.close()


def test_window_past_the_file(cluster):
    smc, files, paths = cluster
    sf = SyncFs(smc.client_conf())
    try:
        r = SyncLocalReader(sf.call(sf.fs.client.open(paths[0])))
        try:
            with pytest.raises(err.OutOfRange):
                r.resolve_token_windows([(len(files[0]) - 10, 0)], "U16", 5,
                                        False)
            groups, slow = r.resolve_token_windows(
                [(len(files[0]) - 12, 0)], "U16", 5, False)
            assert sum(p[3] for _a, ps in groups for p in ps) + \
                sum(s[3] for s in slow) == 6
        finally:
            r.close()
    finally:
        sf.shutdown()
