"""Token documents on the MI355X: the summary / offsets / write kernels
behind native.token_docs on cuda tensors over the case matrix of
token_doc_cases, the argument errors (buffers untouched afterwards), and
CurvineTokenLoader with `documents` over HBM-tier files and over MEM-tier
files with cuda destinations.  Comparisons are exact."""
import numpy as np
import pytest
import torch

from curvine_amd import errors as err
from curvine_amd import native
from curvine_amd.client.filesystem import SyncFs
from curvine_amd.sdk import CurvineTokenLoader
from curvine_amd.testing import SyncMiniCluster
from curvine_amd.testing import test_conf as make_conf

import token_doc_cases as dc
import token_window_cases as tc

pytestmark = pytest.mark.gpu

D = native.DTYPES
DEV = 0
BLOCK = 64
E2E_EOS = 0


def chunk():
    return native.load().TOKEN_DOC_CHUNK


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_sizes(dt):
    dc.case_sizes(native.token_docs, D, DEV, dt, chunk())


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_phases(dt):
    dc.case_phases(native.token_docs, D, DEV, dt, chunk())


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_chunk_edges(dt):
    dc.case_chunk_edges(native.token_docs, D, DEV, dt, chunk())


@pytest.mark.parametrize("dt", dc.DTYPES)
def test_single_outputs(dt):
    dc.case_single_outputs(native.token_docs, D, DEV, dt, chunk())


def test_full_width():
    dc.case_full_width(native.token_docs, D, DEV, chunk())


def test_long_table():
    dc.case_long_table(native.token_docs, D, DEV, chunk())


def test_rejects():
    # pointers on the host side with device 0
    host = torch.full((4096 + 1024,), dc.SENTINEL, dtype=torch.uint8)
    hp = (host.data_ptr() + 4096 + 15) // 16 * 16
    i64 = D["I64"]
    extra = [("x on the host", i64, 3, 8, dc.EOS, hp, 0, 0, 0),
             ("pos on the host", i64, 3, 8, dc.EOS, 0, hp, 0, 0),
             ("doc on the host", i64, 3, 8, dc.EOS, 0, 0, hp, 0),
             ("cu on the host", i64, 3, 8, dc.EOS, 0, 0, 0, hp)]
    dc.run_rejects(native.token_docs, D, DEV, pytest.raises, extra)
    assert bool((host == dc.SENTINEL).all())


def test_rejects_device_pointer_on_the_host():
    x = np.full((3, 8), dc.EOS, np.int64)
    for k in range(4):
        bufs = [dc.Buf(0 if i == k else -1, 25 if i == 3 else 24,
                       4 if i == 3 else 8) for i in range(4)]
        bufs[0].put(x)
        with pytest.raises(ValueError):
            native.token_docs(-1, bufs[0].ptr, 3, 8, D["I64"], dc.EOS,
                              bufs[1].ptr, bufs[2].ptr, bufs[3].ptr)
        bufs[0].expect(x, "x")
        for b in bufs[1:]:
            b.expect(np.zeros(0, np.uint8), "output")


# -------------------------------------------------------------- end to end

def test_end_to_end_hbm_and_mem(tmp_path, monkeypatch):
    files = tc.e2e_files()
    X = tc.e2e_reference(files)[0]
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

        calls = []
        orig = native.token_docs

        def spy(*a, **kw):
            calls.append(a)
            return orig(*a, **kw)
        monkeypatch.setattr(native, "token_docs", spy)

        def maker(paths):
            def make(**kw):
                args = dict(seq_len=tc.E2E["T"], batch_size=tc.E2E["batch"],
                            device="cuda:0", src_dtype=tc.E2E["src"],
                            header_bytes=tc.E2E["header"], drop_last=False)
                args.update(kw)
                ld = CurvineTokenLoader(smc.client_conf(), paths, **args)
                made.append(ld)
                return ld
            return make

        n_batches = -(-len(X) // tc.E2E["batch"])
        for paths in (hbm, mem):            # device kernel, then the slow path
            del calls[:]
            dc.check_doc_loader(maker(paths), X, E2E_EOS, "cuda",
                                tc.E2E["batch"])
            assert len(calls) == 5 * n_batches
            assert all(a[0] == 0 for a in calls)

        ld = maker(hbm)(out_dtype=torch.int32, eos_id=E2E_EOS,
                        documents=dc.DOCS)
        x, _y, docs = next(iter(ld))
        ref = tc.e2e_reference(files, "I32")[0][:len(x)]
        assert np.array_equal(x.cpu().numpy(), ref)
        dc.check_docs(docs, ref, E2E_EOS, dc.DOCS, torch.int32, "cuda")

        dc.check_doc_loader_errors(
            maker(hbm), lambda: pytest.raises(err.InvalidArgument))
    finally:
        for ld in made:
            ld.close()
        if sf is not None:
            sf.shutdown()
        smc.stop()
