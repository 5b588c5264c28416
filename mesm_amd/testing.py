"""Hooks that exist for the test suite only; nothing in the product imports this module."""
import contextlib

from . import kernels, ops
from ._lib import lib


@contextlib.contextmanager
def no_relu():
    """Every ReLU of the Linear blocks bypassed while the context is open: the kink control run of
    tests/test_model_gpu.py compares full-width gradients with the oracle (its NO_RELU switch) on a step that has no
    activation kink to flip."""
    ops._NO_RELU = True
    try:
        yield
    finally:
        ops._NO_RELU = False


@contextlib.contextmanager
def gemm_forced(tile):
    """MESM_GEMM_TILE = tile while the context is open (the library reads the variable once, when it is loaded, so setting
    it in a running process selects nothing): every GEMM launch goes to that kernel, or, where the kernel cannot take it,
    falls through to the automatic choice.  The value that was in force comes back on exit."""
    before = int(lib().mesm_gemm_get_force_tile())
    kernels.gemm_switches(tile=tile)
    try:
        yield
    finally:
        kernels.gemm_switches(tile=before)
