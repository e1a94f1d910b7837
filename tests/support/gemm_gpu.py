"""what tests/test_gemm_edges_gpu.py and tests/test_gemm_mx_edges_gpu.py share: the GEMM launch options put back behind a block, sentinel-filled outputs, raw bits"""
import contextlib

import torch

from oracle import gemm_fp64 as G

BF = torch.bfloat16
_DEFAULTS = (("UTX_GEMM_TILE", 0), ("UTX_GEMM_FASTK", 1), ("UTX_GEMM_STREAMK", 1), ("UTX_GEMM_PERS_GRID", 0), ("UTX_GEMM_GROUP_M", 0))


@contextlib.contextmanager
def _options(**kw):
    """UTX_GEMM_<name> = value inside the block; every GEMM option back at its default behind it, whatever happened"""
    from unitex_amd import _lib
    try:
        for k, v in kw.items():
            _lib.set_option("UTX_GEMM_" + k, int(v))
        yield
    finally:
        for k, v in _DEFAULTS:
            _lib.set_option(k, v)


def _sent(rows, cols):
    return torch.full((rows, cols), G.SENT16, dtype=torch.int16).view(BF)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy()
