"""Token documents without a GPU: token_docs_host (device -1) over the case
matrix of token_doc_cases on CPU tensors, the argument errors (buffers
untouched afterwards), and CurvineTokenLoader with `documents` over MEM-tier
files with device="cpu".  Expected values come from numpy only; comparisons
are exact."""
import pytest

from curvine_amd import errors as err
from curvine_amd import native
from curvine_amd.client.filesystem import SyncFs
from curvine_amd.sdk import CurvineTokenLoader
from curvine_amd.testing import SyncMiniCluster
from curvine_amd.testing import test_conf as make_conf

import token_doc_cases as dc
import token_window_cases as tc

D = native.DTYPES
DEV = -1
BLOCK = 64
E2E_EOS = 0


def chunk():
    return native.load().TOKEN_DOC_CHUNK


def test_chunk_constant():
    assert chunk() >= 256 and chunk() % 64 == 0


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
    dc.run_rejects(native.token_docs, D, DEV, pytest.raises)


# -------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def cluster(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("tokdocs"))
    smc = SyncMiniCluster(conf=make_conf(tmp), tmp_dir=tmp).start()
    sf = SyncFs(smc.client_conf())
    files = tc.e2e_files()
    paths = []
    for i, blob in enumerate(files):
        paths.append(f"/tok/f{i}.bin")
        sf.write_file(paths[-1], blob, storage_tier="MEM", block_size=BLOCK)
    yield smc, files, paths
    sf.shutdown()
    smc.stop()


def maker(smc, paths, made, device):
    def make(**kw):
        args = dict(seq_len=tc.E2E["T"], batch_size=tc.E2E["batch"],
                    device=device, src_dtype=tc.E2E["src"],
                    header_bytes=tc.E2E["header"], drop_last=False)
        args.update(kw)
        ld = CurvineTokenLoader(smc.client_conf(), paths, **args)
        made.append(ld)
        return ld
    return make


def test_end_to_end_mem(cluster, monkeypatch):
    smc, files, paths = cluster
    calls = []
    orig = native.token_docs

    def spy(*a, **kw):
        calls.append(a)
        return orig(*a, **kw)
    monkeypatch.setattr(native, "token_docs", spy)
    made = []
    try:
        X = tc.e2e_reference(files)[0]
        make = maker(smc, paths, made, "cpu")
        dc.check_doc_loader(make, X, E2E_EOS, "cpu", tc.E2E["batch"])
        # one call per batch with documents, on the host, none without
        n_batches = -(-len(X) // tc.E2E["batch"])
        assert len(calls) == 5 * n_batches
        assert all(a[0] == -1 for a in calls)

        import torch
        import numpy as np
        ld = make(out_dtype=torch.int32, eos_id=E2E_EOS, documents=dc.DOCS)
        x, _y, docs = next(iter(ld))
        ref = tc.e2e_reference(files, "I32")[0][:len(x)]
        assert np.array_equal(x.numpy(), ref)
        dc.check_docs(docs, ref, E2E_EOS, dc.DOCS, torch.int32, "cpu")
    finally:
        for ld in made:
            ld.close()


def test_loader_document_errors(cluster):
    smc, _files, paths = cluster
    made = []
    try:
        dc.check_doc_loader_errors(
            maker(smc, paths, made, "cpu"),
            lambda: pytest.raises(err.InvalidArgument))
    finally:
        for ld in made:
            ld.close()
