"""An exact Gram matrix of small integers, for moment tests on dyadic data (entries k / 8, |k| <= 32).

K'K in int64 is exact as long as no sum passes 2^63; numpy multiplies int64 matrices without BLAS (16 s for 40,002 x 227), so the product
is taken in row blocks: a block's product in float64 -- every partial sum of a block is an integer below rows x max|k|^2 <= 2^53, which
float64 represents exactly whatever the order of summation -- converted to int64 and added up in int64.  tests/test_gram_form_cpu.py holds
this against numpy's own int64 product."""
import numpy as np

BLOCK = 4096


def exact_gram(k):
    """k: n x m integer array.  Returns k.T @ k as int64, exactly."""
    k = np.ascontiguousarray(k, dtype=np.int64)
    n, m = k.shape
    amax = int(np.abs(k).max()) if k.size else 0
    assert BLOCK * amax * amax < 2 ** 53 and n * amax * amax < 2 ** 62
    g = np.zeros((m, m), dtype=np.int64)
    for r in range(0, n, BLOCK):
        b = k[r:r + BLOCK].astype(np.float64)
        g += (b.T @ b).astype(np.int64)
    return g
