"""A numpy restatement of the composed moment buffers of the many-response call (oem_amd/csrc/multi.hip, include/oemgpu.h:
oemgpu_selftest_multi_moments_dev), and of the rules its host plan must obey.

Buffer r is the moment buffer about 0 of Z = [x | Y[:, 0] | 1] with the three kinds of entry that depend on the response -- M[p, j] = sum_i
x_ij y_ir, M[p, p] = sum_i y_ir^2, M[p + 1, p] = sum_i y_ir -- and their mirror images replaced by response r's: the Gram block, the column
sums and the row count are those of the one moment pass."""
import numpy as np

ENGINE_ROWS, ENGINE_COOP = 1, 2          # OEMGPU_ENGINE_ROWS, OEMGPU_ENGINE_COOP
MAX_INSTANCES = 513


def composed_moments(x, Y, dtype=np.float64):
    """[m, p + 2, p + 2], indexed [r, i, j] = M_r[i, j]"""
    x = np.asarray(x, dtype=dtype)
    Y = np.asarray(Y, dtype=dtype)
    n, p = x.shape
    m = Y.shape[1]
    z = np.concatenate([x, Y[:, :1], np.ones((n, 1), dtype=dtype)], axis=1)
    base = z.T @ z
    out = np.empty((m, p + 2, p + 2), dtype=dtype)
    for r in range(m):
        M = base.copy()
        xy = x.T @ Y[:, r]
        M[p, :p] = xy
        M[:p, p] = xy
        M[p, p] = Y[:, r] @ Y[:, r]
        M[p + 1, p] = M[p, p + 1] = Y[:, r].sum()
        out[r] = M
    return out


def coop_workgroups(q):
    """path_coop.hip: workgroups of one cooperating set"""
    return (q + 31) // 32 if q <= 512 else (q + 15) // 16


def waiting_workgroups(q, npen, engine, cap, num_cu):
    """Workgroups of ONE batched launch of `cap` instances that wait for each other (0: none do).  q <= 208: one workgroup per instance
    and penalty, which waits for nobody; the four-workgroup form of path_small.hip at 208 < q <= 288 always splits the penalties; the
    cooperating engine splits them while instances x penalties x workgroups stay within half the CUs (paths.hip: pen_split)."""
    if engine == ENGINE_ROWS:
        return 0 if q <= 208 else 4 * npen * cap
    if engine == ENGINE_COOP:
        w = coop_workgroups(q)
        split = npen > 1 and w * npen * cap <= num_cu // 2
        return w * cap * (npen if split else 1)
    return 0
