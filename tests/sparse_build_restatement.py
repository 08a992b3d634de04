"""A numpy restatement of oem_amd/csrc/sparse_build.hip (test infrastructure, no GPU): the plan of oemgpu_sparse_x_create_dev as DESIGN.md
3.17 states it, and the build as the kernels make it -- the line number of every non-zero, the passes of the least-significant-digit
counting sort on the index (per-workgroup digit counts, the scan over (digit, workgroup), the stable scatter), and the other
orientation's pointers by one lower bound per line over the sorted indices."""
import numpy as np

CSC, CSR = 0, 1
MAX_DIGIT_BITS = 11
PER_MIN = 8 * 256          # a workgroup's share: a multiple of eight tiles of 256 non-zeros
CHUNK = 8192               # rows per chunk of the compressed-column kernels (cptr)


def _r256(b):
    return (b + 255) // 256 * 256


def plan(n, p, nnz, layout, num_cu):
    T = n if layout == CSC else p
    key_bits = 0
    while (1 << key_bits) < T:
        key_bits += 1
    passes = max(1, -(-key_bits // MAX_DIGIT_BITS))
    digit_bits = max(1, -(-key_bits // passes))
    want = 4 * num_cu
    per = max(PER_MIN, -(-(-(-nnz // want)) // PER_MIN) * PER_MIN)
    nwg = max(1, -(-nnz // per))
    ne = nnz + 1
    ws = _r256(64) + 2 * _r256(4 * ne)                                   # the flag words, the line numbers, the sorted indices
    for b in range(2):                                                   # ping from two passes on, pong from three
        if passes >= b + 2:
            ws += 2 * _r256(4 * ne) + _r256(8 * ne)
    ws += _r256(4 * (1 << digit_bits) * nwg) + _r256(4 * (1 << digit_bits))
    chunks = (n + CHUNK - 1) // CHUNK
    handle = (_r256(8 * (p + 1)) + 2 * (_r256(4 * ne) + _r256(8 * ne)) + _r256(8 * (n + 1)) + _r256(4 * (chunks + 1) * p))
    return {"passes": passes, "digit_bits": digit_bits, "nwg": nwg, "ws_bytes": ws, "handle_bytes": handle, "per": per, "key_bits": key_bits,
            "T": T}


def _pass(key, payload, shift, digit_bits, per, nwg):
    """one pass as the three kernels make it: tab[d][w], its scan over w, the scan over d, the stable scatter of every workgroup"""
    nnz, nbins = len(key), 1 << digit_bits
    dig = (key.astype(np.int64) >> shift) & (nbins - 1)
    tab = np.zeros((nbins, nwg), np.int64)
    for w in range(nwg):
        tab[:, w] = np.bincount(dig[w * per:(w + 1) * per], minlength=nbins)
    tot = tab.sum(axis=1)
    before_wg = np.cumsum(tab, axis=1) - tab
    before_bin = np.cumsum(tot) - tot
    pos = np.zeros(nnz, np.int64)
    for w in range(nwg):
        d = dig[w * per:(w + 1) * per]
        order = np.argsort(d, kind="stable")                             # rank among the workgroup's non-zeros of the same digit, in order
        cnt = np.bincount(d, minlength=nbins)
        rank = np.empty(len(d), np.int64)
        rank[order] = np.arange(len(d)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        pos[w * per:(w + 1) * per] = before_bin[d] + before_wg[d, w] + rank
    assert len(np.unique(pos)) == nnz and (nnz == 0 or (pos.min() == 0 and pos.max() == nnz - 1))
    out_key = np.empty_like(key)
    out_key[pos] = key
    outs = []
    for a in payload:
        o = np.empty_like(a)
        o[pos] = a
        outs.append(o)
    return out_key, outs


def chunk_ptr(colptr, rowidx, n, p):
    """cptr[c][j]: the entries of column j in rows below c * CHUNK (where column j enters chunk c, counted from the column's start)"""
    chunks = (n + CHUNK - 1) // CHUNK
    col = np.repeat(np.arange(p), np.diff(colptr))
    cptr = np.zeros((chunks + 1, p), np.int32)
    for c in range(chunks + 1):
        cptr[c] = np.bincount(col[np.asarray(rowidx) < c * CHUNK], minlength=p)
    return cptr


def build(layout, ptr, idx, val, n, p, num_cu=256):
    """the handle's arrays from compressed columns (layout CSC) or compressed rows (CSR) whose lines are sorted: a dict with colptr,
    rowidx, val, rowptr, ccol, cval, cptr, maxcol.  Values travel as 64-bit patterns."""
    ptr = np.asarray(ptr, np.int64)
    nnz = int(ptr[-1])
    P = plan(n, p, nnz, layout, num_cu)
    nline, T = (p, n) if layout == CSC else (n, p)
    oidx = np.asarray(idx).astype(np.int32)
    oval = np.asarray(val).astype(np.float64).view(np.uint64) if np.asarray(val).dtype != np.float64 else np.asarray(val).view(np.uint64)
    line = (np.searchsorted(ptr, np.arange(nnz), side="right") - 1).astype(np.int32)      # the last line that starts at or before k
    key, pay = oidx, [line, oval]
    for ps in range(P["passes"]):
        key, pay = _pass(key, pay, ps * P["digit_bits"], P["digit_bits"], P["per"], P["nwg"])
    tptr = np.searchsorted(key, np.arange(T + 1), side="left").astype(np.int64)
    tidx, tval = pay
    own, other = (ptr, oidx, oval.view(np.float64)), (tptr, tidx, tval.view(np.float64))
    (colptr, rowidx, v), (rowptr, ccol, cv) = (own, other) if layout == CSC else (other, own)
    cptr = chunk_ptr(colptr, rowidx, n, p)
    return {"colptr": colptr, "rowidx": rowidx, "val": v, "rowptr": rowptr, "ccol": ccol, "cval": cv, "cptr": cptr,
            "maxcol": int(np.max(np.diff(colptr))) if p > 0 else 0}


def from_scipy(x):
    """what the handle of a scipy matrix holds, by scipy's own conversions (sorted indices)"""
    import scipy.sparse as sp
    n, p = x.shape
    c = sp.csc_matrix(x, dtype=np.float64); c.sort_indices()
    r = sp.csr_matrix(x, dtype=np.float64); r.sort_indices()
    cptr = chunk_ptr(c.indptr, c.indices, n, p)
    return {"colptr": c.indptr.astype(np.int64), "rowidx": c.indices.astype(np.int32), "val": c.data, "rowptr": r.indptr.astype(np.int64),
            "ccol": r.indices.astype(np.int32), "cval": r.data, "cptr": cptr, "maxcol": int(np.max(np.diff(c.indptr)))}


def same(a, b):
    """every array equal, values as bit patterns"""
    for k in ("colptr", "rowidx", "rowptr", "ccol", "cptr"):
        if not np.array_equal(np.asarray(a[k]), np.asarray(b[k])):
            return k
    for k in ("val", "cval"):
        if not np.array_equal(np.ascontiguousarray(a[k], np.float64).view(np.int64), np.ascontiguousarray(b[k], np.float64).view(np.int64)):
            return k
    return None if a["maxcol"] == b["maxcol"] else "maxcol"
