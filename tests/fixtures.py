"""Fixtures that several test files use under one name (TEST HELPER), imported by name into the files that use them:
pytest then treats each as that file's own module-scoped fixture."""
import pytest


@pytest.fixture(scope="module")
def ops():
    """vdr.ops, for GPU tests"""
    import torch
    import vdr  # noqa: F401
    from vdr import ops as _ops
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return _ops


@pytest.fixture(scope="module")
def lib():
    """the loaded C library"""
    from vdr import _lib
    return _lib.load()
