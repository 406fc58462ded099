import os
import sys

import pytest
# torch brings its own HIP runtime, which the native library shares only when torch is loaded first (the library asks for
# libamdhip64.so.7, torch's copy carries that soname; loaded the other way round, the process ends up with two HIP runtimes and
# the library's sees no device).  CPU tests load the library without torch, so torch goes first for the whole session.
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


@pytest.fixture(scope="session")
def reference():
    from oracle.pyoracle import Reference, build
    build()
    if not Reference.available():
        pytest.skip("oracle/_ref/libtsq_ref.so not built (no /root/reference here)")
    return Reference()
