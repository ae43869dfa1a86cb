"""Online sessions without a GPU: the new translation unit is built, the header declares the entries at ABI 9, the binding matches."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "poi_hip.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def _prototype(name):
    m = re.search(r"^int %s\((.*?)\);" % name, _header(), re.S | re.M)
    assert m, "%s is not declared in include/poi_hip.h" % name
    return [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_build_lists_the_session_unit():
    import poi_amd
    assert "session.hip" in poi_amd.build.SOURCES
    assert os.path.exists(os.path.join(poi_amd.build.CSRC, "session.hip"))


def test_header_declares_the_entries_at_abi_9():
    h = _header()
    assert re.search(r"#define POI_ABI_VERSION 9\b", h)
    assert "additive to 9: online sessions" in h
    args = _prototype("poi_session_advance")
    assert args[0] == "poi_ctx* ctx" and args[1] == "const poi_gru_params* prm" and args[-1] == "void* stream"
    for name in ("double* h", "float* sts", "int32_t* last_poi", "int32_t* steps", "int32_t n_slot", "const int32_t* slot", "const int32_t* poi", "float* hts_out", "float* sts_out"):
        assert name in args, name
    assert _prototype("poi_session_sts")[-1] == "void* stream"
    for key in ("session_path", "session_tiles", "session_tile_min"):
        assert '"%s"' % key in h


def test_binding_matches_the_header():
    import poi_amd
    L = poi_amd._lib
    assert L.ABI_VERSION == 9
    for name in ("poi_session_advance", "poi_session_sts"):
        assert name in L.SIGNATURES, name
        assert len(L.SIGNATURES[name][1]) == len(_prototype(name)), name
    for key in ("session_path", "session_tiles", "session_tile_min"):
        assert key in L.PLAN_KEYS


def test_models_expose_the_session():
    import poi_amd
    M = poi_amd.models
    assert callable(M.Session)
    for cls in (M.OboSpatialGru, M.OboGru, M.Gru):
        assert callable(getattr(cls, "session"))
    assert callable(poi_amd.harness.serve_replay)
