"""Online sessions of Lstm / Rnn / CA-RNN without a GPU: the new translation unit is built, the header declares the two entries at ABI 9,
the binding matches, the models expose `cell_session`, and the oracle-side condition that keeps the CA-RNN parity test from running
blind holds (tests/session_cells_oracle.py)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "poi_hip.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def _prototype(name):
    m = re.search(r"^int %s\((.*?)\);" % name, _header(), re.S | re.M)
    assert m, "%s is not declared in include/poi_hip.h" % name
    return [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_build_lists_the_session_cells_unit():
    import poi_amd
    assert "session_cells.hip" in poi_amd.build.SOURCES
    assert os.path.exists(os.path.join(poi_amd.build.CSRC, "session_cells.hip"))


def test_header_declares_both_entries_at_abi_9():
    assert re.search(r"#define POI_ABI_VERSION 9\b", _header())
    assert _prototype("poi_session_cell_advance") == [
        "poi_ctx* ctx", "const poi_cell_params* prm", "double* h", "double* c", "int32_t* last_poi", "int32_t* steps", "int32_t n_slot",
        "const int32_t* slot", "const int32_t* poi", "int32_t n", "float* hts_out", "void* stream"]
    assert _prototype("poi_session_carnn_advance") == [
        "poi_ctx* ctx", "const poi_carnn_params* prm", "const double* coords", "const double* cphi", "const double* thr", "double dd",
        "double* h", "int32_t* last_poi", "int32_t* steps", "int32_t n_slot", "const int32_t* slot", "const int32_t* poi", "int32_t n",
        "float* hts_out", "void* stream"]


def test_binding_matches_the_header():
    import poi_amd
    L = poi_amd._lib
    assert L.ABI_VERSION == 9
    for name in ("poi_session_cell_advance", "poi_session_carnn_advance"):
        assert name in L.SIGNATURES, name
        assert len(L.SIGNATURES[name][1]) == len(_prototype(name)), name


def test_models_expose_cell_session():
    import poi_amd
    M = poi_amd.models
    assert issubclass(M.CellSession, M.Session)
    for cls in (M.Lstm, M.Rnn, M.OboCARNN):
        assert callable(getattr(cls, "cell_session"))
    for cls in (M.OboGru, M.Gru, M.OboSpatialGru):
        assert not hasattr(cls, "cell_session")


@pytest.mark.parametrize("n_dist", [11, 200])
@pytest.mark.parametrize("dim", [8, 20, 64, 128])
def test_carnn_states_saturate_under_the_reference_init_and_not_under_the_shifted_one(dim, n_dist):
    """The problems of the GPU parity test, on the oracle alone: under the reference's init no entry of any FINAL state lies in
    (0.05, 0.95) - a final-state comparison would see nothing; under the shifted init at least 15 % of the (user, prefix) states are
    informative."""
    from tests import session_cells_oracle as S
    from tests.test_gpu_session import geo_problem, seq_bins, seqs_of
    T = geo_problem(300 + dim + n_dist, n_user=24, n_item=50, n_dist=n_dist, dim=dim, len_min=4, len_max=12)
    ref = S.carnn_params(dim, T, shifted=False)
    fin = np.array([S.carnn_prefix_states(ref, q, seq_bins(T, q))[-1] for q in seqs_of(T)])
    assert not ((fin > 0.05) & (fin < 0.95)).any(), "the reference init was expected to saturate every final state"
    P = S.carnn_params(dim, T)
    st = np.concatenate([S.carnn_prefix_states(P, q, seq_bins(T, q)) for q in seqs_of(T)])
    share = float(S.informative(st).mean())
    print("dim %d bins %d: %.1f %% of the prefix states are informative" % (dim, n_dist, 100 * share))
    assert share >= S.INFORMATIVE_MIN
