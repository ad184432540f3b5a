"""Shapes and inputs of the bf16-rounding cases of tests/test_row_passes_rest_gpu.py, shared with tests/test_helper_passes_host.py: the
host file measures, on exactly these inputs, how often a float32 replay rounds to another bf16 value than the float64 reference."""
import numpy as np

PN_PAD_SHAPES = [(1, 1, 32), (3, 5, 96), (2, 16, 1024), (1, 3, 20)]       # (H, W, C)
MEAN3_SHAPES = [(1, 4, 4), (7, 32, 32), (5, 36, 64), (300, 64, 64)]       # (rows, C, ldb)
MEAN3_SLOPES = [0.1, 0.01]


def pn_pad_input(H, W, C):
    """f32 [H][W][C], 3 z; the last position is all zeros (the 1e-6 under the root keeps it finite) when there is more than one"""
    x = (3.0 * np.random.default_rng(H * 100000 + W * 2000 + C).standard_normal((H, W, C))).astype(np.float32)
    if H * W > 1:
        x[-1, -1, :] = 0.0
    return x


def mean3_inputs(rows, C):
    """three f32 [rows][C], 2 z each"""
    rng = np.random.default_rng(rows * 1000 + C)
    return [(2.0 * rng.standard_normal((rows, C))).astype(np.float32) for _ in range(3)]
