"""CPU: origin_glr_plan_prepare -- the norm cube and the eps of a weighted plan ahead of its first
band -- is declared in include/origin_hip.h, exported by liborigin_hip.so and bound by _capi with
the (context, plan) signature GLRPlan.prepare calls it with."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from origin_amd import build, _capi
    build.build()
    return _capi.load()


def test_prepare_is_declared_exported_and_bound(lib):
    from origin_amd import _capi, kernels
    text = open(os.path.join(ROOT, "include", "origin_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+origin_glr_plan_prepare\s*\(\s*origin_ctx\s*\*\s*\w+\s*,\s*"
                     r"origin_glr_plan\s*\*\s*\w+\s*\)\s*;", text)
    raw = ctypes.CDLL(os.path.join(ROOT, "origin_amd", "liborigin_hip.so"))
    for name in ("origin_glr_plan_prepare", "origin_glr_rows_supported", "origin_glr_run_rect"):
        assert hasattr(raw, name), f"{name} is not exported"
    assert _capi.SIGNATURES["origin_glr_plan_prepare"] == [_capi.vp, _capi.vp]
    assert lib.origin_glr_plan_prepare.argtypes == [_capi.vp, _capi.vp]
    assert callable(kernels.GLRPlan.prepare)
