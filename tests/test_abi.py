"""CPU checks of the drop-in boundary: libwafer_hip.so loads and exports exactly what
include/wafer_hip.h declares; the ctypes table matches the header; no compute is launched."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "wafer_hip.h"


def _declared():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decls = {}
    for m in re.finditer(r"\b(?:int|size_t|const char\s*\*)\s+(wm_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        args = [a.strip() for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        decls[m.group(1)] = len(args)
    return decls


@pytest.fixture(scope="module")
def lib():
    from ssl_wafermap_amd import _lib

    if not _lib.LIB_PATH.exists():
        from importlib import import_module

        import_module("ssl_wafermap_amd.build").build(verbose=False)
    return _lib.load()


def test_header_declares_entry_points():
    d = _declared()
    for name in ("wm_version", "wm_augment_views", "wm_knn_topk", "wm_ntxent_fwd", "wm_ntxent_bwd"):
        assert name in d


def test_library_exports_every_declared_symbol(lib):
    for name in _declared():
        assert hasattr(lib, name), f"libwafer_hip.so does not export {name}"


def test_ctypes_table_matches_header(lib):
    from ssl_wafermap_amd import _lib

    d = _declared()
    assert set(d) == set(_lib.SIGNATURES), set(d) ^ set(_lib.SIGNATURES)
    for name, nargs in d.items():
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


def test_version_and_error_strings(lib):
    from ssl_wafermap_amd import _lib

    assert lib.wm_version() == 4
    assert b"unsupported" in lib.wm_error_string(-2)
    with pytest.raises(_lib.WaferHipError):
        _lib.check(-1, "probe")


def test_struct_layout_matches_header():
    from ssl_wafermap_amd import _lib
    from ssl_wafermap_amd.transforms.augmentations import PARAM_DTYPE

    assert ctypes.sizeof(_lib.WmViewParams) == 64 == PARAM_DTYPE.itemsize
    assert [f[0] for f in _lib.WmViewParams._fields_] == list(PARAM_DTYPE.names)
    for name, _ in _lib.WmViewParams._fields_:
        assert getattr(_lib.WmViewParams, name).offset == PARAM_DTYPE.fields[name][1]


def test_argument_validation_needs_no_gpu(lib):
    # null pointers / bad sizes are rejected before any launch
    assert lib.wm_knn_topk(None, None, 1, 1, 128, 0, 1, 0, None, None, None, 0, None) == -1
    assert lib.wm_knn_topk_workspace_bytes(64, 1000, 128, 99) == 0
    assert lib.wm_knn_topk_workspace_bytes(64, 1000, 128, 5) > 0
    assert lib.wm_ntxent_fwd(None, None, 4, 4, 0, 128, 0.5, None, None, None) == -1


def test_conv_route_query_needs_no_gpu(lib, monkeypatch):
    """wm_conv2d_route names the kernel instantiation of every shape of tests/conv_cases.py (the GPU tests of
    csrc/conv.hip ask it again before they launch), refuses what the entry points refuse, and launches nothing."""
    import conv_cases as cc
    import kernel_check as kc

    monkeypatch.delenv("WM_WGRAD_PATCH", raising=False)
    for route, shape in cc.FWD:
        assert lib.wm_conv2d_route(0, *cc.geom(shape), 0, 0) == route, ("fwd", shape)
    for route, shape, groups in cc.FWD_STATS:
        g = cc.geom(shape)
        assert lib.wm_conv2d_route(0, *g, kc.ROUTE_F_STATS, g[0] * g[7] * g[8] // groups) == route, ("fwd stats", shape)
    for route, shape in cc.DGRAD:
        for flags in (0, kc.ROUTE_F_RESIDUAL):
            assert lib.wm_conv2d_route(1, *cc.geom(shape), flags, 0) == route, ("dgrad", shape, flags)
    for route, shape, groups in cc.DGRAD_BNB:
        for flags in (kc.ROUTE_F_BNB, kc.ROUTE_F_BNB | kc.ROUTE_F_RESIDUAL):
            assert lib.wm_conv2d_dgrad_bnstat_ok(*cc.geom(shape), groups) == 1
            assert lib.wm_conv2d_route(1, *cc.geom(shape), flags, groups) == route, ("dgrad bnb", shape, flags)
    assert lib.wm_conv2d_dgrad_bnstat_ok(*cc.geom(cc.BNB_REFUSED), 1) == 0
    assert lib.wm_conv2d_route(1, *cc.geom(cc.BNB_REFUSED), kc.ROUTE_F_BNB, 1) == -2
    for route, g, splits in cc.WGRAD:
        assert lib.wm_conv2d_route(2, *g, 0, 0) == route, ("wgrad", g)
        assert splits is None or lib.wm_conv2d_wgrad_splits(*g) == splits, ("wgrad splits", g)
    for route, shape in cc.WGRAD_STEM:
        assert lib.wm_conv2d_route(2, *cc.geom(shape), 0, 0) == route, ("stem wgrad", shape)
    monkeypatch.setenv("WM_WGRAD_PATCH", "0")
    for route, g in cc.WGRAD_PATCH_OFF:
        assert lib.wm_conv2d_route(2, *g, 0, 0) == route, ("wgrad, patch kernel off", g)
    monkeypatch.delenv("WM_WGRAD_PATCH")
    # the epilogue forms of the Linear layers and the hand-off to the panel kernel
    lin = cc.linear_geom
    assert lib.wm_conv2d_route(0, *lin(129, 64, 128), kc.ROUTE_F_BIAS | kc.ROUTE_F_RESIDUAL, 0) == kc.route_igemm(128, 8, 0, epi=True)
    assert lib.wm_conv2d_route(0, *lin(129, 64, 192), kc.ROUTE_F_BIAS | kc.ROUTE_F_ACT, 0) == kc.route_igemm(64, 8, 0, epi=True)
    assert lib.wm_conv2d_route(1, *lin(129, 64, 128), kc.ROUTE_F_ACT, 0) == kc.route_igemm(64, 8, 3, epi=True)
    assert lib.wm_conv2d_route(0, *lin(129, 192, 384), kc.ROUTE_F_BIAS, 0) == kc.ROUTE_PANEL
    assert lib.wm_conv2d_route(0, *lin(129, 192, 384), kc.ROUTE_F_RESIDUAL, 0) == kc.route_igemm(128, 8, 0, epi=True)
    assert lib.wm_conv2d_route(1, *lin(129, 384, 192), 0, 0) == kc.ROUTE_PANEL
    assert lib.wm_conv2d_route(2, *lin(129, 64, 128), kc.ROUTE_F_BIAS, 0) == kc.route_wgrad(128, 8, 1, bias=True)
    # refused as the entry points refuse: bad sizes, channels, a bias gradient on the patch-resident or stem form,
    # an input gradient of the stem, statistics groups that are no whole tiles, unknown passes and flags
    g = cc.geom((2, 64, 8, 8, 64, 3, 1, 1))
    assert lib.wm_conv2d_route(0, 0, *g[1:], 0, 0) == -1
    assert lib.wm_conv2d_route(0, *cc.geom((1, 32, 8, 8, 64, 3, 1, 1)), 0, 0) == -2
    assert lib.wm_conv2d_route(2, *g, kc.ROUTE_F_BIAS, 0) == -2
    assert lib.wm_conv2d_route(2, *cc.geom(cc.STEM_PATCH_SHAPES[0]), kc.ROUTE_F_BIAS, 0) == -2
    assert lib.wm_conv2d_route(1, *cc.geom(cc.STEM_PATCH_SHAPES[0]), 0, 0) == -2
    assert lib.wm_conv2d_route(0, *g, kc.ROUTE_F_STATS, 100) == -2
    assert lib.wm_conv2d_route(0, *g, kc.ROUTE_F_STATS, 0) == -1
    assert lib.wm_conv2d_route(3, *g, 0, 0) == -1
    assert lib.wm_conv2d_route(0, *g, 64, 0) == -1


def test_product_path_fails_loudly_without_gpu_tensors():
    import torch

    from ssl_wafermap_amd import _lib
    from ssl_wafermap_amd import functional as F

    with pytest.raises(_lib.WaferHipError):
        F.knn_topk(torch.zeros(4, 128), torch.zeros(16, 128), 2)


def test_missing_library_is_an_error(tmp_path):
    from ssl_wafermap_amd import _lib

    with pytest.raises(_lib.WaferHipError):
        _lib.load(tmp_path / "nope.so")


def test_library_sources_issue_no_memset():
    """A hipMemsetAsync captured as a memset node inside the training step's hipGraph was the root cause of the
    round-1 NaN (profiles/r02_nan_root_cause.md): buffers are cleared by kernels (csrc/common.h wm_zero_async)."""
    import re

    csrc = ROOT / "self-supervised-wafermaps_amd" / "csrc"
    for f in sorted(csrc.glob("*.hip")) + sorted(csrc.glob("*.h")):
        code = re.sub(r"//[^\n]*", "", f.read_text())
        assert "hipMemset" not in code, f"{f.name} calls hipMemset*"
