"""Host-side mirror of the reference's R front ends for the dense Gaussian path.

    oem()      <-> R/oem.R:162-507      (.Call("oem_fit_dense", ...)  R/oem.R:556-575)
    oem_xtx()  <-> R/oem_xtx.R:109-360  (.Call("oem_xtx", ...)        R/oem_xtx.R:389-406)
    big_oem()  <-> R/big_oem.R:121-441  (.Call("oem_fit_big", ...)    R/big_oem.R:447-491)

Same argument names (dots become underscores, `lambda` is `lambda_`), same defaults, same
validation messages, same result structure (`beta` / `lambda` / `niter` / `loss` lists, one entry
per penalty, plus `d`, `nobs`, `nvars`, `penalty`, `family`, `varnames`, `nzero`).  All numerics run
in liboemgpu.so (HIP kernels); there is no CPU fallback.

x may be a numpy array (host: the drop-in entry points upload it) or a CUDA/HIP torch tensor
(device resident: the *_dev entry points are used and X is never copied to the host).
"""
import ctypes as C
import warnings

import numpy as np

from . import _lib as L

PENALTIES = L.PENALTIES


class OemFit(dict):
    """The list returned by oem()/oem.xtx()/big.oem() (classes "oemfit_gaussian", "oem")."""

    r_class = ("oemfit_gaussian", "oem")

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


# ------------------------------------------------------------------------------------------ helpers
def _match_penalty(penalty):
    """match.arg(penalty, several.ok=TRUE) (R/oem.R:202-208): default is the first choice only."""
    if penalty is None:
        return [PENALTIES[0]]
    if isinstance(penalty, str):
        penalty = [penalty]
    out = []
    for q in penalty:
        hits = [c for c in PENALTIES if c == q] or [c for c in PENALTIES if c.startswith(q)]
        if len(hits) != 1:
            raise ValueError("'arg' should be one of " + ", ".join(f"'{c}'" for c in PENALTIES))
        out.append(hits[0])
    return out


def _is_torch_cuda(x):
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def _is_scipy_sparse(x):
    return type(x).__module__.startswith("scipy.sparse")


def _is_torch_sparse(x):
    """a torch tensor of any sparse layout (host or device)"""
    if not type(x).__module__.startswith("torch") or not hasattr(x, "layout"):
        return False
    import torch
    return isinstance(x, torch.Tensor) and x.layout != torch.strided


def _torch_sparse_parts(x):
    """The component tensors of a 2-d torch sparse tensor as (layout code, pointers, indices, values), where it lies: compressed rows
    or columns as they are; a COO tensor coalesced by torch (on its device) and its row pointers made with dense ops (bincount,
    cumsum) -- no torch sparse-library call.  ValueError, naming the cause, for a block layout, more than two dimensions, dense
    (hybrid) dimensions and a dtype that is not served."""
    import torch
    if x.layout not in (torch.sparse_csr, torch.sparse_csc, torch.sparse_coo):
        raise ValueError(f"a sparse tensor of layout {x.layout} is not served: torch.sparse_csr, torch.sparse_csc or torch.sparse_coo")
    if x.ndim != 2:
        raise ValueError(f"x must be a matrix: a 2-d sparse tensor, not one of {x.ndim} dimensions")
    n = int(x.shape[0])
    if x.dtype not in (torch.float64, torch.float32):
        raise ValueError(f"the values of a sparse tensor must be float64 or float32, not {x.dtype}")
    if x.layout == torch.sparse_coo:
        if x.dense_dim() != 0:
            raise ValueError("a hybrid sparse tensor (dense dimensions) is not served")
        x = x.coalesce()                                               # sorted by (row, column), duplicates summed: on the tensor's device
        ind, val = x.indices(), x.values()
        ptr = torch.zeros(n + 1, dtype=torch.int64, device=ind.device)
        if ind.shape[1] > 0:
            ptr[1:] = torch.cumsum(torch.bincount(ind[0], minlength=n), 0)
        layout, idx = L.OEMGPU_SPARSE_CSR, ind[1]
    elif x.layout == torch.sparse_csr:
        layout, ptr, idx, val = L.OEMGPU_SPARSE_CSR, x.crow_indices(), x.col_indices(), x.values()
    else:
        layout, ptr, idx, val = L.OEMGPU_SPARSE_CSC, x.ccol_indices(), x.row_indices(), x.values()
    if val.ndim != 1:
        raise ValueError("a hybrid sparse tensor (dense dimensions) is not served")
    if val.dtype not in (torch.float64, torch.float32):
        raise ValueError(f"the values of a sparse tensor must be float64 or float32, not {val.dtype}")
    for t in (ptr, idx):
        if t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"the indices of a sparse tensor must be int32 or int64, not {t.dtype}")
    return layout, ptr.contiguous(), idx.contiguous(), val.contiguous()


def _torch_sparse_to_scipy(x):
    """A sparse torch tensor ON THE HOST as the scipy matrix of its component arrays (values float64; float32 widened)"""
    import scipy.sparse as sp
    if x.is_cuda:
        raise ValueError("a device tensor stays on its device: SparseX(x) takes it there")
    layout, ptr, idx, val = _torch_sparse_parts(x)
    cls = sp.csr_matrix if layout == L.OEMGPU_SPARSE_CSR else sp.csc_matrix
    return cls((val.numpy().astype(np.float64), idx.numpy(), ptr.numpy()), shape=(int(x.shape[0]), int(x.shape[1])))


def _sparse_tensor_arg(x):
    """What a front end makes of its x: a sparse torch tensor on the host becomes its scipy matrix (the scipy route); anything else,
    a sparse device tensor among it, is returned as it is"""
    if _is_torch_sparse(x) and not x.is_cuda:
        return _torch_sparse_to_scipy(x)
    return x


def _csc_arrays(x):
    """The compressed-column arrays of a scipy.sparse x as R's coercion to dgCMatrix leaves them: float64 values, duplicate entries
    summed, row indices sorted inside every column.  Returns contiguous (int64 colptr, int32 rowidx, float64 values).  The caller's
    matrix is never changed: when it is not already in that form, a copy is."""
    import scipy.sparse as sp
    xc = sp.csc_matrix(x, dtype=np.float64)
    if not xc.has_canonical_format:
        xc = xc.copy()
        xc.sum_duplicates()                                            # sums, and sorts the indices
    return (np.ascontiguousarray(xc.indptr, dtype=np.int64), np.ascontiguousarray(xc.indices, dtype=np.int32),
            np.ascontiguousarray(xc.data, dtype=np.float64))


def _dptr(a):
    return a.ctypes.data_as(L._dp) if a is not None and a.size > 0 else L._dp()


def _iptr(a):
    return a.ctypes.data_as(L._ip) if a is not None and a.size > 0 else L._ip()


class _Args:
    """Builds oemgpu_opts and keeps the numpy buffers alive."""

    def __init__(self, penalty, lam_list, nlambda, lambda_min_ratio, alpha, gamma, tau, tol, maxit, accelerate,
                 compute_loss, penalty_factor, groups, unique_groups, group_weights, device=-1, ngpus=0, devices=None,
                 upload_threads=0, interrupt=None):
        self.pen = np.array([PENALTIES.index(q) for q in penalty], dtype=np.int32)
        self.pf = np.ascontiguousarray(penalty_factor, dtype=np.float64)
        nlu = len(lam_list[0]) if lam_list else 0
        self.lam = np.ascontiguousarray(np.stack(lam_list), dtype=np.float64) if nlu > 0 else None
        self.groups = np.ascontiguousarray(groups, dtype=np.int32)
        self.ug = np.ascontiguousarray(unique_groups, dtype=np.int32)
        self.gw = np.ascontiguousarray(group_weights, dtype=np.float64)
        o = L.OemgpuOpts()
        o.npen = len(self.pen); o.penalty = _iptr(self.pen)
        o.nlambda = int(nlambda); o.lambda_min_ratio = float(lambda_min_ratio)
        o.lambda_user = _dptr(self.lam); o.nlambda_user = nlu
        o.alpha, o.gamma, o.tau, o.tol = float(alpha), float(gamma), float(tau), float(tol)
        o.maxit, o.accelerate, o.compute_loss = int(maxit), int(bool(accelerate)), int(bool(compute_loss))
        o.penalty_factor = _dptr(self.pf)
        o.groups = _iptr(self.groups); o.ngroupvars = self.groups.size
        o.unique_groups = _iptr(self.ug); o.ngroups = self.ug.size
        o.group_weights = _dptr(self.gw); o.n_group_weights = self.gw.size
        o.device = int(device)
        # host-resident entry points: rows over `ngpus` devices inside the library (include/oemgpu.h)
        self.devices = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        o.ngpus = int(ngpus) if self.devices is None else len(self.devices)
        o.devices = _iptr(self.devices) if self.devices is not None else None
        o.upload_threads = int(upload_threads)
        if interrupt is not None:
            self._cb = L.OemgpuOpts._fields_[-2][1](lambda _arg: int(bool(interrupt())))      # kept alive with the struct
            o.interrupt = self._cb
        self.c = o
        self.nl = nlu if nlu > 0 else int(nlambda)
        self.npen = len(self.pen)

    def subset(self, idx):
        """the penalties idx of this call as a call of their own (penalties are independent cold starts,
        ref src/oem_dense.cpp:206-246): same options, their rows of a user-supplied lambda"""
        o = self.c
        sub = _Args([PENALTIES[self.pen[k]] for k in idx], [] if self.lam is None else [self.lam[k] for k in idx], o.nlambda,
                    o.lambda_min_ratio, o.alpha, o.gamma, o.tau, o.tol, o.maxit, o.accelerate, o.compute_loss, self.pf,
                    self.groups, self.ug, self.gw, device=o.device)
        return sub

    def outputs(self, rows):
        self.beta = np.zeros((self.npen, self.nl, rows))
        self.lam_out = np.zeros((self.npen, self.nl))
        self.niter = np.zeros((self.npen, self.nl), dtype=np.int32)
        self.loss = np.zeros((self.npen, self.nl))
        self.d = C.c_double(0.0)
        return [_dptr(self.beta), _dptr(self.lam_out), _iptr(self.niter), _dptr(self.loss), C.byref(self.d)]


def _lambda_list(lambda_, npen):
    """R/oem.R:366-404"""
    if isinstance(lambda_, (list, tuple)) and len(lambda_) > 0 and np.ndim(lambda_[0]) > 0:
        if len(lambda_) != npen:
            raise ValueError("If list of lambda vectors is provided, it must be \n"
                             "                  the same length as the number of penalties fit")
        n0 = len(lambda_[0])
        out = []
        for l in lambda_:
            if l is None or len(l) < 1:
                raise ValueError("Provided lambda vector must have at least one value")
            if len(l) != n0:
                raise ValueError("All provided lambda vectors must have same length")
            out.append(np.sort(np.asarray(l, dtype=np.float64))[::-1].copy())
        return out
    lam = np.sort(np.asarray(lambda_, dtype=np.float64).ravel())[::-1].copy()
    return [lam.copy() for _ in range(npen)]


def _group_setup(penalty, groups, group_weights, p, intercept_adds_zero_group):
    """R/oem.R:287-338 (dense gaussian: the intercept never adds a group) and R/big_oem.R:226-259."""
    if any("grp" in q for q in penalty):
        groups = np.asarray(groups).ravel()
        if len(groups) != p:
            raise ValueError("If any group penalty is used groups must have same length as number of columns in x")
        unique_groups = np.sort(np.unique(groups))
        has_zero = bool(np.any(unique_groups == 0))
        if group_weights is not None:
            group_weights = np.asarray(group_weights, dtype=np.float64).ravel().copy()
            # `group.weights[zero.idx] <- 0` indexes with the VALUE 0, a no-op in R: kept as is
            if not has_zero and intercept_adds_zero_group:
                unique_groups = np.concatenate([[0], unique_groups])
                group_weights = np.concatenate([[0.0], group_weights])
            if len(group_weights) != len(unique_groups):
                raise ValueError("group.weights must have same length as the number of groups")
        else:
            group_weights = np.zeros(0)
            if not has_zero and intercept_adds_zero_group:
                unique_groups = np.sort(np.concatenate([[0], unique_groups]))
        if intercept_adds_zero_group:
            groups = np.concatenate([[0], groups])
        return groups.astype(np.int32), unique_groups.astype(np.int32), group_weights
    return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)


def _common_checks(nlambda, lambda_min_ratio, maxit, irls_maxit, tol, irls_tol):
    if lambda_min_ratio >= 1 or lambda_min_ratio <= 0:
        raise ValueError("lambda.min.ratio must be between 0 and 1")
    if int(np.ravel(nlambda)[0]) <= 0:
        raise ValueError("nlambda must be a positive integer")
    if maxit <= 0 or irls_maxit <= 0:
        raise ValueError("maxit and irls.maxit should be positive")
    if tol < 0 or irls_tol < 0:
        raise ValueError("tol and irls.tol should be nonnegative")


def _nonzero_lists(beta, zero_first_row=True):
    """predict.oem(type="nonzero") (R/methods.R:93-100): row 1 is always treated as the intercept (quirk Q16)."""
    b = np.array(beta, copy=True)
    if zero_first_row:
        b[0, :] = 0
    return [np.nonzero(np.abs(b[:, j]) > 0)[0] + 1 if np.any(np.abs(b[:, j]) > 0) else None for j in range(b.shape[1])]


def _decorate(a, penalty, varnames, intercept_row, n, p, family="gaussian"):
    """R/oem.R:487-507"""
    res = OemFit()
    res["beta"], res["lambda"], res["niter"], res["loss"] = [], [], [], []
    for k, name in enumerate(penalty):
        b = a.beta[k].T.copy()                       # rows x nl
        if name == "ols":                            # quirk Q9: vector reshaped to a 1-column matrix
            res["beta"].append(b[:, :1]); res["niter"].append(int(a.niter[k, 0])); res["loss"].append(float(a.loss[k, 0]))
        else:
            res["beta"].append(b); res["niter"].append(a.niter[k].copy()); res["loss"].append(a.loss[k].copy())
        res["lambda"].append(a.lam_out[k].copy())
    res["d"] = a.d.value
    res["rownames"] = (["(Intercept)"] if intercept_row else []) + list(varnames)
    # sapply(predict.oem(type = "nonzero"), length): row 1 is always dropped as "the intercept" (quirk Q16)
    res["nzero"] = [(np.abs(np.asarray(b)[1:]) > 0).sum(axis=0) for b in res["beta"]]
    if n is not None:
        res["nobs"] = n
    res["nvars"] = p
    res["penalty"] = list(penalty)
    res["family"] = family
    res["varnames"] = list(varnames)
    return res


def _device_matrix(x):
    """(data_ptr, n, p, ld, keepalive) of a torch device matrix in column-major order."""
    import torch
    if x.dtype != torch.float64:
        x = x.to(torch.float64)
    n, p = x.shape
    if x.stride(0) == 1 and x.stride(1) >= n:           # already column-major
        return x.data_ptr(), n, p, x.stride(1), x
    xt = x.t().contiguous()                              # (p, n) row-major == (n, p) column-major
    return xt.data_ptr(), n, p, n, xt


def _rowmajor_dtype(x):
    """OEMGPU_F64 / OEMGPU_F32 for a torch tensor the row-major entries can read in place (unit column stride, row stride >= p,
    float64 or float32), else None."""
    import torch
    code = {torch.float64: L.OEMGPU_F64, torch.float32: L.OEMGPU_F32}.get(x.dtype)
    if code is None or x.ndim != 2 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        return None
    return code


def _rowmajor_in_place(x):
    """The dtype code with which oem() hands a device tensor to oemgpu_fit_dense_rm_dev as it lies, or None: then _device_matrix
    makes the column-major float64 copy (p >= n, p beyond the row-major pass, a tensor that is already column-major or strided in
    its columns, other element types)."""
    n, p = x.shape
    if n <= p or p > L.RM_P_MAX:
        return None
    if x.stride(0) == 1 and x.stride(1) >= n:                          # already column-major (_device_matrix takes it without a copy)
        return None
    return _rowmajor_dtype(x)


def _logistic_rowmajor_in_place(x):
    """The dtype code with which the binomial entries (oem_fit_logistic_dense, its fold form, logistic_cv_score, cv_oem(family=
    "binomial")) hand a device tensor to their _rm_dev entry as it lies, or None: then it goes the column-major way (a tensor that is
    already column-major, one strided in its columns, other element types)."""
    if x.ndim == 2 and x.stride(0) == 1 and x.stride(1) >= x.shape[0]:   # already column-major (_device_matrix takes it without a copy)
        return None
    return _rowmajor_dtype(x)


def _xval_rowmajor_in_place(x):
    """The dtype code with which xval_oem and the fold fits of cv_oem(family="gaussian") hand a device tensor to their _rm_dev entry as
    it lies, or None: then it goes the column-major way.  _logistic_rowmajor_in_place's rule -- not already column-major, unit column
    stride, a row stride of at least p, float64 or float32 -- and no limit on p: the rows are gathered into fold order, and the moment
    passes run on that copy."""
    return _logistic_rowmajor_in_place(x)


class _DeviceX:
    """A torch device matrix as the C entries take it.  `policy` (_rowmajor_in_place, _logistic_rowmajor_in_place or
    _xval_rowmajor_in_place) says whether the _rm_dev entry reads x where it lies -- `code` is then its dtype code, `ld` the row stride
    -- or the _dev entry reads a column-major float64 matrix (_device_matrix: x itself, or the one copy): `code` is None, `ld` the
    column stride.  `keep` holds the memory behind `ptr`; `resident` is the n x p tensor over it."""

    def __init__(self, x, policy):
        self.code = policy(x)
        if self.code is None:
            self.ptr, self.n, self.p, self.ld, self.keep = _device_matrix(x)
        else:
            (self.n, self.p), self.ptr, self.ld, self.keep = x.shape, x.data_ptr(), x.stride(0), x

    @property
    def resident(self):                                                # (made when asked for: a torch call per fit is host time per fit)
        if self.code is not None:
            return self.keep
        return self.keep.as_strided((self.n, self.p), (1, self.ld), self.keep.storage_offset())

    def call(self, stem, ctx, *rest):
        """oemgpu_<stem>_dev(ctx, x, n, ld, p, *rest), or oemgpu_<stem>_rm_dev(ctx, x, dtype, n, ldr, p, *rest) on a row-major x"""
        if self.code is None:
            return L.check(getattr(L.lib(), f"oemgpu_{stem}_dev")(ctx, self.ptr, self.n, self.ld, self.p, *rest))
        return L.check(getattr(L.lib(), f"oemgpu_{stem}_rm_dev")(ctx, self.ptr, self.code, self.n, self.ld, self.p, *rest))


def _device_y(y, device):
    """y as a contiguous float64 device vector: a host y goes to `device`, a device tensor stays where it is"""
    import torch
    yd = y if _is_torch_cuda(y) else torch.as_tensor(np.asarray(y, dtype=np.float64), device=device)
    return yd.to(torch.float64).contiguous().reshape(-1)


def _rowmajor_args(x, y):
    if not _is_torch_cuda(x):
        raise ValueError("x must be a torch tensor on a GPU")
    code = _rowmajor_dtype(x)
    if code is None:
        raise ValueError("x must be float64 or float32 with unit column stride and a row stride of at least p")
    n, p = x.shape
    yd = _device_y(y, x.device)
    if yd.shape[0] != n:
        raise ValueError("x and y lengths do not match")
    return code, n, p, yd


def rowmajor_shift_sums(x, y):
    """Test infrastructure: oemgpu_shift_sums_rm_dev on a row-major device tensor x (float64 / float32, read in place) -> the sums
    buffer as a numpy array (include/oemgpu.h: oemgpu_sums_len)."""
    import torch
    code, n, p, yd = _rowmajor_args(x, y)
    sums = torch.empty(L.sums_len(p), dtype=torch.float64, device=x.device)
    ctx = context(x.device.index)
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_shift_sums_rm_dev(ctx, x.data_ptr(), code, n, x.stride(0), p, yd.data_ptr(), sums.data_ptr()))
    L.check(L.lib().oemgpu_synchronize(ctx))
    return sums.cpu().numpy()


def rowmajor_moments(x, y, sums=None):
    """Test infrastructure: oemgpu_moments_rm_dev on a row-major device tensor x -> the (p + 2) x (p + 2) moment buffer about the shift
    `sums` defines (a sums buffer as rowmajor_shift_sums returns it; None: about 0), as a numpy array indexed [i, j] = M[i, j]."""
    import torch
    code, n, p, yd = _rowmajor_args(x, y)
    mom = torch.empty(L.moments_len(p), dtype=torch.float64, device=x.device)
    sd = None if sums is None else torch.as_tensor(np.ascontiguousarray(sums, dtype=np.float64), device=x.device)
    ctx = context(x.device.index)
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_moments_rm_dev(ctx, x.data_ptr(), code, n, x.stride(0), p, yd.data_ptr(), None if sd is None else sd.data_ptr(),
                                          mom.data_ptr()))
    L.check(L.lib().oemgpu_synchronize(ctx))
    return mom.cpu().numpy().reshape(p + 2, p + 2).T


def rowmajor_fold_order(x, y, foldid, nfolds):
    """Test infrastructure: oemgpu_selftest_fold_gather_rm_dev on a row-major device tensor x (float64 / float32, read in place) -> (xo,
    yo, fold_n, fold_start): the fold-ordered rows as numpy arrays xo[position, column] and yo[position] over every position of the
    layout (NaN where nothing was written) and the folds' sizes and first positions."""
    import torch
    code, n, p, yd = _rowmajor_args(x, y)
    K = int(nfolds)
    fd = torch.as_tensor(np.ascontiguousarray(foldid, dtype=np.int32), device=x.device)
    if fd.shape[0] != n:
        raise ValueError("x and foldid lengths do not match")
    ldo = (n + 16 * K + 15) // 16 * 16
    xo = torch.full((p, ldo), float("nan"), dtype=torch.float64, device=x.device)
    yo = torch.full((ldo,), float("nan"), dtype=torch.float64, device=x.device)
    fold_n, fold_start = np.zeros(max(K, 1), dtype=np.int64), np.zeros(max(K, 1), dtype=np.int64)
    ctx = context(x.device.index)
    torch.cuda.current_stream(x.device).synchronize()
    i64 = C.POINTER(C.c_int64)
    L.check(L.lib().oemgpu_selftest_fold_gather_rm_dev(ctx, x.data_ptr(), code, n, x.stride(0), p, yd.data_ptr(), fd.data_ptr(), K, xo.data_ptr(),
                                                       ldo, yo.data_ptr(), fold_n.ctypes.data_as(i64), fold_start.ctypes.data_as(i64)))
    L.check(L.lib().oemgpu_synchronize(ctx))
    return xo.cpu().numpy().T, yo.cpu().numpy(), fold_n, fold_start


_ctx_cache = {}


ENGINES = ("none", "rows", "coop", "rowcoop", "symcoop", "launches", "wcoop", "wres", "wstream", "wlaunches", "sparse-wide")   # OEMGPU_ENGINE_* (include/oemgpu.h)


def last_path_engine(ctx=None):
    """(name of the kernel family that ran the most recent penalty x lambda path on this context, number of persistent-engine calls
    so far that timed out and were made again with launches) -- for device-resident inputs, whose calls run on `context()`."""
    e, f = C.c_int32(0), C.c_int32(0)
    L.check(L.lib().oemgpu_last_path_engine(ctx if ctx is not None else context(), C.byref(e), C.byref(f)))
    return ENGINES[e.value], f.value


def last_host_path_engine():
    """name of the kernel family that ran the calling thread's most recent penalty x lambda path, on whatever context -- for host
    inputs (numpy, scipy.sparse), whose calls run on a context of the library's own (include/oemgpu.h: oemgpu_last_host_path_engine)."""
    e = C.c_int32(0)
    L.check(L.lib().oemgpu_last_host_path_engine(C.byref(e)))
    return ENGINES[e.value]


def last_path_rounds(ctx=None):
    """(short_rounds, rounds) of the most recent path on the row-split kernel (include/oemgpu.h: oemgpu_last_path_rounds)."""
    s, r = C.c_int64(0), C.c_int64(0)
    L.check(L.lib().oemgpu_last_path_rounds(ctx if ctx is not None else context(), C.byref(s), C.byref(r)))
    return int(s.value), int(r.value)


def last_placement(ctx=None):
    """"none" / "one-xcd" / "refused": whether the cooperating engine of the most recent path launch on this context ran with all
    workgroups of an instance on one XCD (include/oemgpu.h: oemgpu_last_placement)."""
    return ("none", "one-xcd", "refused", "crowded")[L.lib().oemgpu_last_placement(ctx if ctx is not None else context())]


def context(device=None, stream=None):
    """A cached oemgpu_ctx per (device, stream).  stream: a torch.cuda.Stream or None (own stream)."""
    import torch
    if device is None:
        device = torch.cuda.current_device()
    sptr = None if stream is None else int(stream.cuda_stream)
    key = (int(device), sptr)
    if key not in _ctx_cache:
        h = L.lib().oemgpu_create(int(device), C.c_void_p(sptr) if sptr else None)
        if not h:
            raise L.OemgpuError(-2, L.lib().oemgpu_last_error().decode())
        _ctx_cache[key] = h
    return _ctx_cache[key]


# ------------------------------------------------------------------------------------------ oem()
def _fit_options(n, p, penalty, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups, penalty_factor, group_weights, maxit, tol,
                 irls_maxit, irls_tol, varnames, zero_group, groups_sentence=False, accelerate=False, compute_loss=False, **device):
    """The option prologue of every fit entry behind its checks of x and y (R/oem.R:268-404, R/oem_xtx.R:180-300, R/big_oem.R:200-330,
    R/oem_xval.R:225-330) -> (_Args, varnames).  What differs between the entries is in the arguments (the table in DESIGN.md 1):
    zero_group, whether the intercept adds group 0 (_group_setup); groups_sentence, whether the length of `groups` has a sentence of its
    own before _group_setup; accelerate and compute_loss, which some entries fix; **device, the ngpus / devices / upload_threads /
    interrupt that the entry has."""
    if penalty_factor is None:
        penalty_factor = np.ones(p)
    penalty_factor = np.asarray(penalty_factor, dtype=np.float64).ravel()
    if varnames is None:
        varnames = [f"V{i + 1}" for i in range(p)]
    if len(penalty_factor) != p:
        raise ValueError("penalty.factor must have same length as number of columns in x")
    if groups_sentence and any("grp" in q for q in penalty) and len(np.ravel(groups)) != p:
        raise ValueError("groups must have same length as number of columns in x")
    groups, unique_groups, group_weights = _group_setup(penalty, groups, group_weights, p, zero_group)
    if lambda_min_ratio is None:
        lambda_min_ratio = 0.01 if n < p else 0.0001
    _common_checks(nlambda, float(lambda_min_ratio), maxit, irls_maxit, tol, irls_tol)
    lam_list = _lambda_list(lambda_, len(penalty))
    a = _Args(penalty, lam_list, int(np.ravel(nlambda)[0]), lambda_min_ratio, alpha, gamma, tau, tol, maxit, accelerate,
              compute_loss, penalty_factor, groups, unique_groups, group_weights, **device)
    return a, varnames


def oem(x, y, family="gaussian", penalty=None, weights=(), lambda_=(), nlambda=100, lambda_min_ratio=None,
        alpha=1.0, gamma=3.0, tau=0.5, groups=(), penalty_factor=None, group_weights=None, standardize=True,
        intercept=True, maxit=500, tol=1e-7, irls_maxit=100, irls_tol=1e-3, accelerate=False, ncores=-1,
        compute_loss=False, hessian_type="upper.bound", varnames=None, ngpus=0, devices=None, upload_threads=0,
        interrupt=None, _entry_weights=None, _args_only=False, _res_fit=False):
    """oem(): R/oem.R:162-507, dense gaussian branch.  ngpus / devices / upload_threads / interrupt: the host-resident
    options of include/oemgpu.h (`options` gains ngpus / device; absent => one GPU).
    A sparse torch tensor (sparse_csr, sparse_csc, sparse_coo) is oem_fit_sparse's: on a device it is fitted where it lies."""
    if _is_torch_sparse(x):
        kw = {k: v for k, v in locals().items() if k not in ("x", "y", "_entry_weights", "_args_only", "_res_fit")}
        return oem_fit_sparse(x, y, **kw)
    L.sync_switches()
    if family not in ("gaussian", "binomial"):
        raise ValueError("'arg' should be one of 'gaussian', 'binomial'")
    penalty = _match_penalty(penalty)
    resident_sparse = isinstance(x, SparseX)
    if resident_sparse and not _args_only:
        if getattr(x, "_h", None) is None:
            raise ValueError("this SparseX is closed")
        if x.shape[0] > x.shape[1] and not _res_fit:                  # n > p through oem() itself: the sentence stays (oem_fit_sparse serves the handle)
            raise ValueError("oem() on a SparseX is not built: oem() takes the scipy.sparse matrix itself; the resident handle is what cv_oem runs on")
    if getattr(x, "ndim", 0) != 2 and not resident_sparse:
        raise ValueError("x must have at least two columns")
    n, p = x.shape
    if p > n:
        warnings.warn("oem() is optimized for n >> p settings and may be very slow when p > n")
    if p < 2:
        raise ValueError("x must have at least two columns")
    is_sparse = type(x).__module__.startswith("scipy.sparse") or resident_sparse      # R/oem.R:236-242: sparseMatrix -> dgCMatrix
    if len(weights) > 0:
        raise ValueError("weights not implemented yet.")
    ylen = y.shape[0] if hasattr(y, "shape") else len(y)
    if ylen != n:
        raise ValueError("x and y lengths do not match")
    if family == "binomial":
        raise NotImplementedError("family='binomial' is outside the dense Gaussian hot path (ref src/oem_logistic_dense.cpp)")
    a, varnames = _fit_options(n, p, penalty, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups, penalty_factor, group_weights,
                               maxit, tol, irls_maxit, irls_tol, varnames, bool(intercept) and is_sparse,                # R/oem.R:296-338
                               accelerate=accelerate, compute_loss=compute_loss, ngpus=ngpus, devices=devices,
                               upload_threads=upload_threads, interrupt=interrupt)
    if _args_only:                                                    # cv_oem's resident route: the option block of this call, nothing run
        if is_sparse:
            a.c.accelerate = 0                                         # oemSparse has no acceleration
        return a, varnames, bool(standardize), bool(intercept)
    lib = L.lib()
    if resident_sparse:                                                # n <= p on the handle: from its non-zeros, nothing uploaded but y
        if ngpus or devices is not None:
            raise ValueError("oem() on a SparseX: the rows of a sparse x are not split over devices")
        a.c.accelerate = 0                                             # oemSparse has no acceleration
        if intercept and n <= p:
            _sparse_wide_intercept_refusal(n, p, a, standardize)
        import torch
        yd = _device_y(y, x.device).to(x.device)
        torch.cuda.current_stream(x.device).synchronize()
        if n > p:                                                      # oem_fit_sparse on the handle: the Gram form from the resident columns
            L.check(lib.oemgpu_fit_sparse_res(context(x.device.index), x.handle, yd.data_ptr(), int(bool(standardize)), int(bool(intercept)),
                                              C.byref(a.c), *a.outputs(p + 1)))
            return _decorate(a, penalty, varnames, True, n, p)
        L.check(lib.oemgpu_fit_sparse_wide_res(context(x.device.index), x.handle, yd.data_ptr(), int(bool(standardize)), C.byref(a.c),
                                               *a.outputs(p + 1)))
        return _decorate(a, penalty, varnames, True, n, p)
    if is_sparse:                                                      # oem_fit_sparse (ref src/oem_sparse.cpp:30-267)
        colptr, rowidx, vals = _csc_arrays(x)
        yh = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        a.c.accelerate = 0                                             # oemSparse has no acceleration
        L.check(lib.oemgpu_fit_sparse(n, p, colptr.ctypes.data, _iptr(rowidx), _dptr(vals), _dptr(yh), int(bool(standardize)),
                                      int(bool(intercept)), C.byref(a.c), *a.outputs(p + 1)))
        return _decorate(a, penalty, varnames, True, n, p)
    if _entry_weights is not None:                                     # oem_fit_dense with a weights vector (oem_fit_dense_weighted below)
        if is_sparse:
            raise ValueError("observation weights: dense x only (oem_fit_sparse ignores its weights argument)")
        wh = np.ascontiguousarray(np.asarray(_entry_weights, dtype=np.float64).reshape(-1))
        if wh.shape[0] != n:
            raise ValueError("length of weights not same as number of observations in x")       # R/oem.R:261-266
        if _is_torch_cuda(x):
            import torch
            xp, n_, p_, ld, keep = _device_matrix(x)
            yd = torch.as_tensor(np.asarray(y.cpu() if _is_torch_cuda(y) else y, dtype=np.float64), device=x.device).reshape(-1)
            wd = torch.as_tensor(wh, device=x.device)
            ctx = context(x.device.index)
            torch.cuda.current_stream(x.device).synchronize()
            L.check(lib.oemgpu_fit_dense_weighted_dev(ctx, xp, n, ld, p, yd.data_ptr(), wd.data_ptr(), int(bool(standardize)),
                                                      int(bool(intercept)), C.byref(a.c), *a.outputs(p + 1)))
            del keep
        else:
            xh = np.asfortranarray(x, dtype=np.float64)
            yh = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
            L.check(lib.oemgpu_fit_dense_weighted(_dptr(xh), n, p, _dptr(yh), _dptr(wh), int(bool(standardize)), int(bool(intercept)),
                                                  C.byref(a.c), *a.outputs(p + 1)))
        return _decorate(a, penalty, varnames, True, n, p)
    if _is_torch_cuda(x):
        import torch
        X = _DeviceX(x, _rowmajor_in_place)                            # read where it lies (no float64 copy, no transposed copy) where that serves
        yd = _device_y(y, x.device)
        ctx = context(x.device.index)
        torch.cuda.current_stream(x.device).synchronize()
        X.call("fit_dense", ctx, yd.data_ptr(), int(bool(standardize)), int(bool(intercept)), C.byref(a.c), *a.outputs(p + 1))
    else:
        xh = np.asfortranarray(x, dtype=np.float64)
        yh = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        L.check(lib.oemgpu_fit_dense(_dptr(xh), n, p, _dptr(yh), int(bool(standardize)), int(bool(intercept)),
                                     C.byref(a.c), *a.outputs(p + 1)))
    return _decorate(a, penalty, varnames, True, n, p)


class _OneOfMany:
    """The outputs of response r of a many-response call, as _decorate reads an _Args"""

    def __init__(self, beta, lam_out, niter, loss, d):
        self.beta, self.lam_out, self.niter, self.loss, self.d = beta, lam_out, niter, loss, C.c_double(float(d))


class _ManyOut:
    """The outputs of a call that makes m fits with the option block `a`: what _Args.outputs allocates, with a leading m"""

    def __init__(self, m, a, rows):
        self.beta = np.zeros((m, a.npen, a.nl, rows))
        self.lam_out = np.zeros((m, a.npen, a.nl))
        self.niter = np.zeros((m, a.npen, a.nl), dtype=np.int32)
        self.loss = np.zeros((m, a.npen, a.nl))
        self.d = np.zeros(m)

    def pointers(self):
        """the five result pointers in the order of the C ABI"""
        return [_dptr(self.beta), _dptr(self.lam_out), _iptr(self.niter), _dptr(self.loss), _dptr(self.d)]

    def one(self, r):
        return _OneOfMany(self.beta[r], self.lam_out[r], self.niter[r], self.loss[r], self.d[r])


def _device_responses(Y, device):
    """Y (n x m) as the many-response entries read it: (tensor, row stride, column stride).  A float64 device tensor with a unit stride
    in one dimension (and the other at least the extent it steps over) is read where it lies; any other device tensor is converted
    once, a host array uploaded once."""
    import torch
    Yd = Y if _is_torch_cuda(Y) else torch.as_tensor(np.ascontiguousarray(np.asarray(Y, dtype=np.float64)), device=device)
    if Yd.device != device:
        Yd = Yd.to(device)
    n, m = Yd.shape
    rs, cs = Yd.stride()
    if Yd.dtype != torch.float64 or not ((cs == 1 and rs >= m) or (rs == 1 and cs >= n)):
        Yd = Yd.to(torch.float64).contiguous()
        rs, cs = Yd.stride()
        if not (cs == 1 and rs >= m):                                  # (n x 1 contiguous has strides (1, 1))
            rs, cs = m, 1
    return Yd, int(rs), int(cs)


def multi_plan(n, p, m, npen=1, layout=0, num_cu=256):
    """oemgpu_selftest_multi_plan (pure host arithmetic) as a dict"""
    out = (C.c_int64 * 8)()
    L.check(L.lib().oemgpu_selftest_multi_plan(int(n), int(p), int(m), int(npen), int(layout), int(num_cu), out))
    keys = ["rows", "row_chunks", "block", "passes", "cap", "solve_chunks", "engine", "bytes"]
    return dict(zip(keys, [int(v) for v in out]))


def multi_moments(x, Y):
    """Test infrastructure: oemgpu_selftest_multi_moments_dev -> the m composed moment buffers, numpy [m, p + 2, p + 2] indexed
    [r, i, j] = M_r[i, j].  x: a torch device tensor, read where it lies when it is column-major float64 or row-major float64 / float32."""
    import torch
    if not _is_torch_cuda(x) or x.ndim != 2:
        raise ValueError("x must be a 2-D torch tensor on a GPU")
    n, p = x.shape
    if x.dtype == torch.float64 and x.stride(0) == 1 and x.stride(1) >= n:
        code, ld = -1, x.stride(1)
    else:
        code, ld = _rowmajor_dtype(x), x.stride(0)
        if code is None:
            raise ValueError("x must be column-major float64, or row-major float64 / float32 with unit column stride")
    Yd, rs, cs = _device_responses(Y, x.device)
    m = Yd.shape[1]
    out = torch.full((m, p + 2, p + 2), float("nan"), dtype=torch.float64, device=x.device)
    ctx = context(x.device.index)
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_selftest_multi_moments_dev(ctx, x.data_ptr(), code, n, ld, p, Yd.data_ptr(), rs, cs, m, out.data_ptr()))
    return out.cpu().numpy().transpose(0, 2, 1).copy()                # (the buffers are column-major)


def oem_multi(x, Y, family="gaussian", weights=(), ngpus=0, devices=None, **kw):
    """m responses on one resident x: [oem(x, Y[:, r], **kw) for r in range(m)] from two reads of x -- one moment pass, one X'Y pass
    (multi.hip) -- and the paths of up to 513 responses per launch (include/oemgpu.h: oemgpu_fit_dense_multi_dev).  x: a torch device
    tensor, n x p with n > p, taken as oem() takes it (row-major float64 / float32 read in place, else column-major float64).
    Y: n x m, a torch device tensor (float64 with a unit stride in one dimension: read where it lies) or a host array (uploaded once).
    oem()'s keyword arguments and checks; a user lambda is shared by all responses.  Returns a list of m OemFit, each with one more key,
    `route`: 0 solved in a batched launch, 1 one by one from its composed moments, 2 fitted again about a shift (oem()'s own route)."""
    if getattr(Y, "ndim", None) != 2:
        raise ValueError("Y must be a matrix of n rows and one column per response")
    if family != "gaussian":
        if family == "binomial":
            raise ValueError("family='binomial' is outside the dense Gaussian hot path (ref src/oem_logistic_dense.cpp)")
        raise ValueError("'arg' should be one of 'gaussian', 'binomial'")
    if len(weights) > 0:
        raise ValueError("weights not implemented yet.")
    if ngpus or devices is not None:
        raise ValueError("oem_multi(): the rows of a resident x are not split over devices (ngpus / devices)")
    host_or_sparse = "oem_multi() takes a dense torch tensor on a GPU: a host or sparse x is fitted one response at a time with oem()"
    if isinstance(x, SparseX) or _is_scipy_sparse(x) or _is_torch_sparse(x):
        raise ValueError(host_or_sparse)
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must have at least two columns")
    n, p = x.shape
    if Y.shape[0] != n:
        raise ValueError("x and y lengths do not match")
    m = int(Y.shape[1])
    if m < 1:
        raise ValueError("Y must have at least one column")
    if n <= p:
        raise ValueError("oem_multi() serves n > p only: with n <= p fit each column with oem(x, Y[:, r])")
    if not _is_torch_cuda(x):
        raise ValueError(host_or_sparse)
    penalty =_match_penalty(kw.pop("penalty", None))
    a, varnames, standardize, intercept = oem(x, Y, penalty=penalty, _args_only=True, **kw)
    import torch
    X = _DeviceX(x, _rowmajor_in_place)
    Yd, rs, cs = _device_responses(Y, x.device)
    out = _ManyOut(m, a, p + 1)
    route = np.zeros(m, dtype=np.int32)
    ctx = context(x.device.index)
    torch.cuda.current_stream(x.device).synchronize()
    X.call("fit_dense_multi", ctx, Yd.data_ptr(), rs, cs, m, int(standardize), int(intercept), C.byref(a.c), *out.pointers(), _iptr(route))
    fits = []
    for r in range(m):
        fit = _decorate(out.one(r), penalty, varnames, True, n, p)
        fit["route"] = int(route[r])
        fits.append(fit)
    return fits


def oem_fit_sparse(x, y, **kw):
    """`.Call("oem_fit_sparse", ...)` (ref src/oem_sparse.cpp:30-267), the entry oem() reaches with a sparse x, with oem()'s arguments
    and result.  x: a scipy.sparse matrix (oem()'s own route: oemgpu_fit_sparse), a SparseX of any shape (oemgpu_fit_sparse_res: the
    moment buffer from the resident columns, nothing uploaded but y; n <= p from the non-zeros, without an intercept), or a sparse
    torch tensor -- on a device it is wrapped in a SparseX for the length of the call, on the host it becomes its scipy matrix.
    y: numpy or a device tensor.  On a handle: no weights, no ngpus / devices."""
    x = _sparse_tensor_arg(x)
    if _is_torch_sparse(x):
        with SparseX(x) as sx:
            return oem(sx, y, _res_fit=True, **kw)
    if isinstance(x, SparseX):
        return oem(x, y, _res_fit=True, **kw)
    if not _is_scipy_sparse(x):
        raise TypeError("x must be a scipy.sparse matrix, a SparseX or a sparse torch tensor (oem takes a dense one)")
    return oem(x, y, **kw)


def oem_fit_dense_weighted(x, y, weights, **kw):
    """What the compiled entry `oem_fit_dense` computes when it is handed a non-empty `weights_` (ref src/oem_dense.cpp:34,75,152,162;
    src/oem_dense.h:368-414, 699-707, 759-770; src/DataStd.h:94-202).  R's oem() stops with "weights not implemented yet" before it
    gets there (R/oem.R:244) and so does `oem()` here; this is the entry below that check, with oem()'s other arguments."""
    return oem(x, y, _entry_weights=weights, **kw)


class OemFitBinomial(OemFit):
    """The list returned by `.Call("oem_fit_logistic_dense", ...)` once oem() has decorated it (class "oemfit_binomial", R/oem.R:582-649)."""

    r_class = ("oemfit_binomial", "oem")


def oem_fit_logistic_dense(x, y, penalty=None, weights=(), lambda_=(), nlambda=100, lambda_min_ratio=None, alpha=1.0, gamma=3.0, tau=0.5,
                           groups=(), penalty_factor=None, group_weights=None, standardize=True, intercept=True, maxit=500, tol=1e-7,
                           irls_maxit=100, irls_tol=1e-3, compute_loss=False, hessian_type="upper.bound", varnames=None, interrupt=None,
                           _fold=None):
    """The dense binomial fit (ref src/oem_logistic_dense.cpp:30-313, src/oem_logistic_dense.h:397-1094) with oem()'s checks for
    family = "binomial" (R/oem.R:162-507): y takes at most two values (passed on as they are: the reference fits the raw 0/1 vector),
    groups gain the intercept's group 0 in front (R/oem.R:296-338).  x: numpy (host entry) or a torch tensor on a GPU (_dev entry; a
    row-major float64 / float32 tensor is read where it lies by the _rm_dev entry, with the column-major fit's bits: DESIGN.md 3.9a).
    hessian_type: "upper.bound" (X'WX, d and A from the first IRLS step of a penalty only) or "full" (every step).  `oem(family=
    "binomial")` still raises NotImplementedError; this is the entry below it, as oem_fit_dense_weighted is for weights.
    _fold (cv_oem's fold fits; x on a GPU): (foldid as an int32 device tensor, nfolds, leave_out, y as a float64 device tensor) -- the
    fit on the rows with foldid != leave_out of the resident x (oemgpu_fit_logistic_dense_fold_dev), which reports their number as nobs."""
    L.sync_switches()
    penalty = _match_penalty(penalty)
    if hessian_type not in ("upper.bound", "full"):
        raise ValueError("'arg' should be one of 'upper.bound', 'full'")
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must have at least two columns")
    n, p = x.shape
    if p < 2:
        raise ValueError("x must have at least two columns")
    if len(weights) > 0:                                               # R/oem.R:244
        raise L.OemgpuError(-4, "weights not implemented yet.")
    yh = np.asarray(y.cpu() if _is_torch_cuda(y) else y, dtype=np.float64).reshape(-1)
    if yh.shape[0] != n:
        raise ValueError("x and y lengths do not match")
    if len(np.unique(yh)) > 2:                                         # R/oem.R:250-252
        raise ValueError("y must be a binary outcome")
    a, varnames = _fit_options(n, p, penalty, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups, penalty_factor, group_weights,
                               maxit, tol, irls_maxit, irls_tol, varnames, bool(intercept), compute_loss=compute_loss, interrupt=interrupt)
    hf = 1 if hessian_type == "full" else 0
    lib = L.lib()
    if _is_torch_cuda(x):
        import torch
        X = _DeviceX(x, _logistic_rowmajor_in_place)                   # row-major float64 / float32: read where it lies
        yd = torch.as_tensor(yh, device=x.device) if _fold is None else _fold[3]
        ctx = context(x.device.index)
        torch.cuda.current_stream(x.device).synchronize()
        scal = (int(bool(standardize)), int(bool(intercept)), hf, int(irls_maxit), float(irls_tol), C.byref(a.c))
        if _fold is None:
            X.call("fit_logistic_dense", ctx, yd.data_ptr(), *scal, *a.outputs(p + 1))
        else:
            fd, nfolds, leave_out = _fold[:3]
            X.call("fit_logistic_dense_fold", ctx, yd.data_ptr(), fd.data_ptr(), int(nfolds), int(leave_out), *scal, *a.outputs(p + 1))
            n = int(n - (fd == int(leave_out)).sum().item())
    else:
        xh = np.asfortranarray(x, dtype=np.float64)
        if _fold is not None:
            raise ValueError("a fold fit needs x on a GPU")
        L.check(lib.oemgpu_fit_logistic_dense(_dptr(xh), n, p, _dptr(yh), int(bool(standardize)), int(bool(intercept)), hf,
                                              int(irls_maxit), float(irls_tol), C.byref(a.c), *a.outputs(p + 1)))
    res = OemFitBinomial(_decorate(a, penalty, varnames, True, n, p, family="binomial"))
    return res


def _binary_columns_check(Y):
    """R/oem.R:250-252 for every column of Y: at most two values.  A device Y is looked at on the device (a column has at most two
    values iff each of its entries equals the column's minimum or its maximum) and never copied to the host."""
    if _is_torch_cuda(Y):
        import torch
        lo, hi = Y.amin(dim=0, keepdim=True), Y.amax(dim=0, keepdim=True)
        bad = torch.nonzero(((Y != lo) & (Y != hi)).any(dim=0)).reshape(-1)          # (a NaN equals neither: its column is named)
        bad = [int(bad[0].item())] if bad.numel() else []
    else:
        Yh = np.asarray(Y, dtype=np.float64)
        bad = [r for r in range(Yh.shape[1]) if len(np.unique(Yh[:, r])) > 2][:1]
    if bad:
        raise ValueError(f"y must be a binary outcome: column {bad[0]} of Y takes more than two values")


def oem_fit_logistic_dense_multi(x, Y, penalty=None, weights=(), lambda_=(), nlambda=100, lambda_min_ratio=None, alpha=1.0, gamma=3.0,
                                 tau=0.5, groups=(), penalty_factor=None, group_weights=None, standardize=True, intercept=True, maxit=500,
                                 tol=1e-7, irls_maxit=100, irls_tol=1e-3, compute_loss=False, hessian_type="upper.bound", varnames=None,
                                 interrupt=None):
    """m binomial responses on one resident x: [oem_fit_logistic_dense(x, Y[:, r], **kw) for r in range(m)] with hessian_type
    "upper.bound", from ONE weighted Gram pass and ONE Lanczos -- at beta = 0 every IRLS weight is 0.25, so X'WX, d and A do not depend
    on y -- and one read of x per IRLS step for all responses that are still iterating (include/oemgpu.h:
    oemgpu_fit_logistic_dense_multi_dev).  x: a dense torch tensor on a GPU with p + intercept <= 1024, taken as
    oem_fit_logistic_dense takes it (row-major float64 / float32 read in place, else column-major float64).  Y: n x m, every column
    with at most two values; a torch device tensor (float64 with a unit stride in one dimension: read where it lies, checked on the
    device) or a host array (uploaded once).  oem_fit_logistic_dense's keyword arguments and checks; a user lambda is shared by all
    responses.  Returns a list of m OemFitBinomial."""
    return _logistic_multi_fit("oem_fit_logistic_dense_multi", x, Y, None, penalty, weights, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups,
                               penalty_factor, group_weights, standardize, intercept, maxit, tol, irls_maxit, irls_tol, compute_loss, hessian_type,
                               varnames, interrupt)


def _logistic_multi_fit(who, x, Y, fold, penalty, weights, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups, penalty_factor, group_weights,
                        standardize, intercept, maxit, tol, irls_maxit, irls_tol, compute_loss, hessian_type, varnames, interrupt):
    """oem_fit_logistic_dense_multi (fold None: one fit per column of Y) and oem_fit_logistic_dense_multi_folds (fold = (foldid,
    instances or None)): the checks, which raise before a device is looked for, then the one call.  Returns the list of fits, one per
    response or per instance."""
    L.sync_switches()
    penalty = _match_penalty(penalty)
    if hessian_type not in ("upper.bound", "full"):
        raise ValueError("'arg' should be one of 'upper.bound', 'full'")
    if getattr(Y, "ndim", None) != 2:
        raise ValueError("Y must be a matrix of n rows and one column per response")
    if len(weights) > 0:                                               # R/oem.R:244
        raise L.OemgpuError(-4, "weights not implemented yet.")
    host_or_sparse = (f"{who}() takes a dense torch tensor on a GPU: a host or sparse x is fitted one response at a "
                      "time with oem_fit_logistic_dense / oem_fit_logistic_sparse")
    if isinstance(x, SparseX) or _is_scipy_sparse(x) or _is_torch_sparse(x):
        raise ValueError(host_or_sparse)
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must have at least two columns")
    n, p = x.shape
    if p < 2:
        raise ValueError("x must have at least two columns")
    if Y.shape[0] != n:
        raise ValueError("x and y lengths do not match")
    m = int(Y.shape[1])
    if m < 1:
        raise ValueError("Y must have at least one column")
    if hessian_type == "full":
        raise ValueError("hessian_type='full' builds one Hessian per response and IRLS step: fit each column with oem_fit_logistic_dense")
    if p + int(bool(intercept)) > 1024:
        raise ValueError(f"{who}() serves p + intercept <= 1024: fit each column with oem_fit_logistic_dense")
    _binary_columns_check(Y)
    if not _is_torch_cuda(x):
        raise ValueError(host_or_sparse)
    resp = leave = None
    if fold is not None:
        foldid, instances = fold
        if _is_torch_cuda(foldid):
            import torch
            if foldid.dtype != torch.int32 or foldid.ndim != 1 or not foldid.is_contiguous():
                raise ValueError("foldid on a device must be a contiguous int32 vector")
            fd, nf_len, nfolds = foldid, int(foldid.shape[0]), (int(foldid.max().item()) if foldid.numel() else 0)
        else:
            fh = np.ascontiguousarray(np.asarray(foldid).ravel(), dtype=np.int32)
            fd, nf_len, nfolds = None, len(fh), (int(fh.max()) if len(fh) else 0)
        if nf_len != n:
            raise ValueError("x and y lengths do not match")
        if nfolds < 3:
            raise ValueError("nfolds must be bigger than 3; nfolds=10 recommended")
        if instances is None:
            instances = [(r, k) for r in range(m) for k in range(nfolds + 1)]
        instances = [(int(r), int(k)) for r, k in instances]
        if len(instances) < 1:
            raise ValueError("instances must name at least one (response, fold) pair")
        for r, k in instances:
            if not 0 <= r < m:
                raise ValueError(f"instance ({r}, {k}): the response must be in [0, {m})")
            if not 0 <= k <= nfolds:
                raise ValueError(f"instance ({r}, {k}): the fold left out must be in [0, {nfolds}] (0: the full fit)")
        resp = np.ascontiguousarray([r for r, _ in instances], dtype=np.int32)
        leave = np.ascontiguousarray([k for _, k in instances], dtype=np.int32)
    a, varnames = _fit_options(n, p, penalty, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups, penalty_factor, group_weights,
                               maxit, tol, irls_maxit, irls_tol, varnames, bool(intercept), compute_loss=compute_loss, interrupt=interrupt)
    import torch
    X = _DeviceX(x, _logistic_rowmajor_in_place)                       # row-major float64 / float32: read where it lies
    Yd, rs, cs = _device_responses(Y, x.device)
    nfit = m if fold is None else len(resp)
    out = _ManyOut(nfit, a, p + 1)
    nobs = np.full(nfit, n, dtype=np.int64)
    ctx = context(x.device.index)
    scal = (int(bool(standardize)), int(bool(intercept)), 0, int(irls_maxit), float(irls_tol), C.byref(a.c))
    outs = out.pointers()
    if fold is None:
        torch.cuda.current_stream(x.device).synchronize()
        X.call("fit_logistic_dense_multi", ctx, Yd.data_ptr(), rs, cs, m, *scal, *outs)
    else:
        if fd is None:
            fd = torch.as_tensor(fh, device=x.device)
        torch.cuda.current_stream(x.device).synchronize()
        X.call("fit_logistic_dense_multi_fold", ctx, Yd.data_ptr(), rs, cs, m, fd.data_ptr(), nfolds, nfit, _iptr(resp), _iptr(leave), *scal, *outs,
               nobs.ctypes.data_as(C.POINTER(C.c_int64)))
    return [OemFitBinomial(_decorate(out.one(r), penalty, varnames, True, int(nobs[r]), p, family="binomial")) for r in range(nfit)]


def oem_fit_logistic_dense_multi_folds(x, Y, foldid, instances=None, penalty=None, weights=(), lambda_=(), nlambda=100, lambda_min_ratio=None, alpha=1.0,
                                       gamma=3.0, tau=0.5, groups=(), penalty_factor=None, group_weights=None, standardize=True, intercept=True,
                                       maxit=500, tol=1e-7, irls_maxit=100, irls_tol=1e-3, compute_loss=False, hessian_type="upper.bound",
                                       varnames=None, interrupt=None):
    """The full and fold fits of a cross-validation over the m columns of Y, from ONE lock-step call on the resident x
    (oemgpu_fit_logistic_dense_multi_fold_dev).  Instance (r, k) is response r fitted on the rows with foldid != k,
    k = 0 the full fit: what oem_fit_logistic_dense(x, Y[:, r]) and its fold form return, with nobs the rows kept.  One Gram pass and
    one Lanczos per distinct k; every instance rides the shared row pass as a masked column.  foldid: n ids in [1, K], a host array or
    an int32 device tensor; K is its largest id.  instances: a list of (r, k) pairs -> the list of their fits, in that order; None: all
    m (K + 1) pairs -> m lists [full, fold 1, ..., fold K].  x, Y and the keyword arguments are oem_fit_logistic_dense_multi's, with its
    checks and refusals; also refused: K < 3, len(foldid) != n, an r outside [0, m), a k outside [0, K], a fold that keeps no more than
    p + intercept rows.  x must be finite on every row, also on rows that only some instances leave out."""
    fits = _logistic_multi_fit("oem_fit_logistic_dense_multi_folds", x, Y, (foldid, instances), penalty, weights, lambda_, nlambda, lambda_min_ratio,
                               alpha, gamma, tau, groups, penalty_factor, group_weights, standardize, intercept, maxit, tol, irls_maxit, irls_tol,
                               compute_loss, hessian_type, varnames, interrupt)
    if instances is not None:
        return fits
    per = len(fits) // int(Y.shape[1])
    return [fits[r * per:(r + 1) * per] for r in range(int(Y.shape[1]))]


def logistic_multi_plan(n, p, m, intercept=True, layout=0, num_cu=256):
    """oemgpu_selftest_logistic_multi_plan (pure host arithmetic) as a dict"""
    out = (C.c_int64 * 16)()
    L.check(L.lib().oemgpu_selftest_logistic_multi_plan(int(n), int(p), int(m), int(bool(intercept)), int(layout), int(num_cu), out))
    keys = ["rows", "row_chunks", "block", "lt", "band", "lds_bytes", "mch", "response_chunks", "blocks", "tiles_per_wave",
            "panel_bytes", "shared_bytes", "chunk_bytes", "hessian_bytes", "bytes", "a_in_lds"]
    return dict(zip(keys, [int(v) for v in out]))


def logistic_multi_stats():
    """oemgpu_last_logistic_multi_stats of this thread, as a dict (the ms are 0 unless the context is timing)"""
    out = (C.c_double * 10)()
    L.check(L.lib().oemgpu_last_logistic_multi_stats(out))
    keys = ["steps", "row_passes", "blocks_skipped", "inner_iters", "grams", "lanczos", "rows_ms", "gram_ms", "inner_ms", "wall_ms"]
    return dict(zip(keys, list(out)))


def logistic_multi_rows(x, Y, btilde=None, intercept=True, mode=1, live=None, out=None):
    """Test infrastructure: oemgpu_selftest_logistic_multi_rows_dev, ONE shared row pass -> numpy [m, p + 2], response r's
    [sum r, X'r, sum of the loss terms].  x: a torch device tensor read where it lies (column-major float64, row-major float64 /
    float32); Y: n x m as _device_responses reads it; btilde: [m, p + intercept] (mode 1); live: m words or None; out: a device
    tensor [m, p + 2] the pass writes the live responses' rows of (default: NaN-filled)."""
    import torch
    if not _is_torch_cuda(x) or x.ndim != 2:
        raise ValueError("x must be a 2-D torch tensor on a GPU")
    n, p = x.shape
    if x.dtype == torch.float64 and x.stride(0) == 1 and x.stride(1) >= n:
        code, ld = -1, x.stride(1)
    else:
        code, ld = _rowmajor_dtype(x), x.stride(0)
        if code is None:
            raise ValueError("x must be column-major float64, or row-major float64 / float32 with unit column stride")
    Yd, rs, cs = _device_responses(Y, x.device)
    m = Yd.shape[1]
    bt = None if btilde is None else torch.as_tensor(np.ascontiguousarray(btilde, dtype=np.float64), device=x.device)
    if out is None:
        out = torch.full((m, p + 2), float("nan"), dtype=torch.float64, device=x.device)
    lv = None if live is None else np.ascontiguousarray(live, dtype=np.int32)
    ctx = context(x.device.index)
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_selftest_logistic_multi_rows_dev(ctx, x.data_ptr(), code, n, ld, p, Yd.data_ptr(), rs, cs, m,
                                                           0 if bt is None else bt.data_ptr(), int(bool(intercept)), int(mode), _iptr(lv),
                                                           out.data_ptr()))
    return out.cpu().numpy()


def logistic_multi_rows_fold(x, Y, foldid, leave, btilde=None, intercept=True, mode=1, live=None, out=None, ycol=None):
    """Test infrastructure: oemgpu_selftest_logistic_multi_rows_fold_dev, ONE masked row pass -> numpy [ncol, p + 2].  Column t is
    response ycol[t] of Y (t itself without ycol) on the rows with foldid != leave[t].  foldid: n ids (host array or int32 device
    tensor); leave, ycol: ncol words; the rest as logistic_multi_rows."""
    import torch
    if not _is_torch_cuda(x) or x.ndim != 2:
        raise ValueError("x must be a 2-D torch tensor on a GPU")
    n, p = x.shape
    if x.dtype == torch.float64 and x.stride(0) == 1 and x.stride(1) >= n:
        code, ld = -1, x.stride(1)
    else:
        code, ld = _rowmajor_dtype(x), x.stride(0)
        if code is None:
            raise ValueError("x must be column-major float64, or row-major float64 / float32 with unit column stride")
    Yd, rs, cs = _device_responses(Y, x.device)
    m = Yd.shape[1]
    fd = foldid if _is_torch_cuda(foldid) else torch.as_tensor(np.ascontiguousarray(foldid, dtype=np.int32), device=x.device)
    if fd.dtype != torch.int32 or fd.shape != (n,) or not fd.is_contiguous():
        raise ValueError("foldid must be n contiguous int32 ids")
    lv = np.ascontiguousarray(leave, dtype=np.int32).ravel()
    ncol = len(lv)
    yc = None if ycol is None else np.ascontiguousarray(ycol, dtype=np.int32).ravel()
    if yc is not None and len(yc) != ncol:
        raise ValueError("ycol and leave must have one entry per column")
    bt = None if btilde is None else torch.as_tensor(np.ascontiguousarray(btilde, dtype=np.float64), device=x.device)
    if bt is not None and bt.shape[0] != ncol:
        raise ValueError("btilde must have one row per column")
    if out is None:
        out = torch.full((ncol, p + 2), float("nan"), dtype=torch.float64, device=x.device)
    lw = None if live is None else np.ascontiguousarray(live, dtype=np.int32)
    ctx = context(x.device.index)
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_selftest_logistic_multi_rows_fold_dev(ctx, x.data_ptr(), code, n, ld, p, Yd.data_ptr(), rs, cs, m, fd.data_ptr(), ncol,
                                                                _iptr(lv), _iptr(yc), 0 if bt is None else bt.data_ptr(), int(bool(intercept)),
                                                                int(mode), _iptr(lw), out.data_ptr()))
    return out.cpu().numpy()


def logistic_multi_fold_plan(n, p, ninst, ngroups, intercept=True, layout=0, num_cu=256):
    """oemgpu_selftest_logistic_multi_fold_plan (pure host arithmetic) as a dict"""
    out = (C.c_int64 * 11)()
    L.check(L.lib().oemgpu_selftest_logistic_multi_fold_plan(int(n), int(p), int(ninst), int(ngroups), int(bool(intercept)), int(layout), int(num_cu), out))
    keys = ["rows", "row_chunks", "chunk_instances", "instance_chunks", "groups", "panel_bytes", "group_bytes", "shared_bytes", "chunk_bytes",
            "hessian_bytes", "bytes"]
    return dict(zip(keys, [int(v) for v in out]))


class SparseX:
    """A scipy.sparse x resident on a GPU (oemgpu_sparse_x_create): the compressed columns as _csc_arrays leaves them, their chunk
    pointers and the compressed-row copy, uploaded and built once.  cv_oem(family="binomial") on a sparse x makes one and runs its full
    fit, its fold fits and its scoring on it; oem_fit_sparse, oem_fit_logistic_sparse, xval_oem, cv_oem, predict and logistic_cv_score
    take one.  Owns the handle: close() frees it (so does leaving a `with` block, and __del__); a closed SparseX refuses further use.
    x may also be a sparse torch tensor (sparse_csr, sparse_csc or sparse_coo; float64 / float32 values, int32 / int64 indices).  On a
    device the handle is built there from the tensor's components (oemgpu_sparse_x_create_dev: checked, copied and transposed in HIP;
    nothing goes to the host; unsorted lines and duplicates are refused, a COO tensor is coalesced by torch first); on the host it
    becomes the scipy matrix of its components.  The handle holds copies: the tensor may be freed afterwards."""

    def __init__(self, x, device=None):
        import scipy.sparse as sp
        import torch
        self._h = None
        if _is_torch_sparse(x):
            if x.is_cuda:
                self._from_device_tensor(x)
                return
            x = _torch_sparse_to_scipy(x)
        if not sp.issparse(x):
            raise TypeError("x must be a scipy.sparse matrix")
        if len(x.shape) != 2:
            raise ValueError("x must have at least two columns")
        self.shape = (int(x.shape[0]), int(x.shape[1]))
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else (torch.device(device).index or 0))
        colptr, rowidx, vals = _csc_arrays(x)
        self.nnz = int(colptr[-1])
        h = C.c_void_p()
        L.check(L.lib().oemgpu_sparse_x_create(context(self.device.index), self.shape[0], self.shape[1], colptr.ctypes.data, _iptr(rowidx),
                                               _dptr(vals), C.byref(h)))
        self._h = h

    def _from_device_tensor(self, x):
        import torch
        layout, ptr, idx, val = _torch_sparse_parts(x)
        self.shape = (int(x.shape[0]), int(x.shape[1]))
        self.device = val.device
        self.nnz = int(val.shape[0])
        code = {torch.int32: L.OEMGPU_I32, torch.int64: L.OEMGPU_I64, torch.float64: L.OEMGPU_F64, torch.float32: L.OEMGPU_F32}
        h = C.c_void_p()
        torch.cuda.current_stream(self.device).synchronize()           # the components (a coalesce, the row pointers) are in place
        L.check(L.lib().oemgpu_sparse_x_create_dev(context(self.device.index), self.shape[0], self.shape[1], layout, ptr.data_ptr(), code[ptr.dtype],
                                                   idx.data_ptr() if self.nnz else None, code[idx.dtype],
                                                   val.data_ptr() if self.nnz else None, code[val.dtype], self.nnz, C.byref(h)))
        self._h = h

    def export(self):
        """oemgpu_sparse_x_export: the handle's arrays on the host, as a dict -- colptr, rowidx, val (compressed columns), rowptr, ccol,
        cval (compressed rows), cptr (the chunk pointers, chunks + 1 rows of p) and maxcol"""
        n, p = self.shape
        dims = (C.c_int64 * 4)()
        L.check(L.lib().oemgpu_sparse_x_dims(self.handle, dims))
        nnz, chunks = int(dims[2]), (n + 8191) // 8192
        out = {"colptr": np.zeros(p + 1, np.int64), "rowidx": np.zeros(nnz, np.int32), "val": np.zeros(nnz, np.float64),
               "rowptr": np.zeros(n + 1, np.int64), "ccol": np.zeros(nnz, np.int32), "cval": np.zeros(nnz, np.float64),
               "cptr": np.zeros((chunks + 1, p), np.int32)}
        L.check(L.lib().oemgpu_sparse_x_export(self.handle, *[out[k].ctypes.data for k in ("colptr", "rowidx", "val", "rowptr", "ccol", "cval", "cptr")]))
        out["maxcol"] = int(dims[3])
        return out

    def to_scipy(self):
        """the matrix as a scipy.sparse.csc_matrix (float64, sorted indices) from the handle's compressed columns"""
        import scipy.sparse as sp
        n, p = self.shape
        colptr, rowidx, val = np.zeros(p + 1, np.int64), np.zeros(self.nnz, np.int32), np.zeros(self.nnz, np.float64)
        L.check(L.lib().oemgpu_sparse_x_export(self.handle, colptr.ctypes.data, rowidx.ctypes.data, val.ctypes.data, None, None, None, None))
        return sp.csc_matrix((val, rowidx, colptr), shape=(n, p))

    @property
    def handle(self):
        if self._h is None:
            raise ValueError("this SparseX is closed")
        return self._h

    @property
    def closed(self):
        return self._h is None

    @property
    def device_bytes(self):
        """the bytes of device memory the handle holds (oemgpu_sparse_x_bytes)"""
        return int(L.lib().oemgpu_sparse_x_bytes(self.handle))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            L.lib().oemgpu_sparse_x_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:                                              # (interpreter shutdown: the library may be gone)
            pass


def oem_fit_logistic_sparse(x, y, penalty=None, weights=(), lambda_=(), nlambda=100, lambda_min_ratio=None, alpha=1.0, gamma=3.0, tau=0.5,
                            groups=(), penalty_factor=None, group_weights=None, standardize=True, intercept=True, maxit=500, tol=1e-7,
                            irls_maxit=100, irls_tol=1e-3, compute_loss=False, hessian_type="upper.bound", varnames=None, interrupt=None,
                            _fold=None):
    """The sparse binomial fit (ref src/oem_logistic_sparse.cpp:30-313, src/oem_logistic_sparse.h), the entry `oem(x = <dgCMatrix>,
    family = "binomial")` calls (R/oem.R:603-624), with the checks of oem_fit_logistic_dense.  x: any scipy.sparse matrix, taken as
    compressed columns of float64 with duplicates summed and indices sorted, as R's coercion to dgCMatrix does.
    hessian_type must be "upper.bound" or "full" and is then ignored: the reference rebuilds X'WX at every IRLS step of this fit
    whatever it says (src/oem_logistic_sparse.h:866, :973).  An intercept needs standardize (the reference's linear predictor reads
    column scales it only computes with standardize); p + intercept >= n is refused.
    _fold (cv_oem's fold fits): (a SparseX, foldid as an int32 device tensor or None, nfolds, leave_out, y as a float64 device tensor) --
    the fit on the rows with foldid != leave_out of the resident x (oemgpu_fit_logistic_sparse_fold_res; leave_out = 0: every row, the
    bits of the plain call), which reports their number as nobs.  x is then not looked at beyond its shape (the SparseX itself may be
    passed).
    x may also be an open SparseX (the fit on the handle: leave_out = 0, the plain call's bits) or a sparse torch tensor: on a device it
    is wrapped in a SparseX for the length of the call, on the host it becomes its scipy matrix.  y: numpy or a device tensor."""
    import scipy.sparse as sp
    x = _sparse_tensor_arg(x)
    if _is_torch_sparse(x):                                            # a sparse device tensor: a SparseX for the length of the call
        kw = {k: v for k, v in locals().items() if k not in ("x", "y", "sp", "_fold")}
        with SparseX(x) as sx:
            return oem_fit_logistic_sparse(sx, y, **kw)
    L.sync_switches()
    penalty = _match_penalty(penalty)
    if hessian_type not in ("upper.bound", "full"):
        raise ValueError("'arg' should be one of 'upper.bound', 'full'")
    if not (sp.issparse(x) or isinstance(x, SparseX)):
        raise TypeError("x must be a scipy.sparse matrix (oem_fit_logistic_dense takes a dense one)")
    if len(x.shape) != 2:
        raise ValueError("x must have at least two columns")
    n, p = x.shape
    if p < 2:
        raise ValueError("x must have at least two columns")
    if len(weights) > 0:                                               # R/oem.R:244
        raise L.OemgpuError(-4, "weights not implemented yet.")
    yh = np.ascontiguousarray(np.asarray(y.cpu() if _is_torch_cuda(y) else y, dtype=np.float64).reshape(-1))
    if yh.shape[0] != n:
        raise ValueError("x and y lengths do not match")
    if len(np.unique(yh)) > 2:                                         # R/oem.R:250-252
        raise ValueError("y must be a binary outcome")
    a, varnames = _fit_options(n, p, penalty, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups, penalty_factor, group_weights,
                               maxit, tol, irls_maxit, irls_tol, varnames, bool(intercept), compute_loss=compute_loss, interrupt=interrupt)
    if _fold is None and isinstance(x, SparseX):                       # the fit on a handle: leave_out = 0, the bits of the plain call
        import torch
        _fold = (x, None, 3, 0, torch.as_tensor(yh, device=x.device))
    if _fold is not None:
        import torch
        sx, fd, nfolds, leave_out, yd = _fold
        if tuple(sx.shape) != (n, p):
            raise ValueError("the SparseX does not have the shape of x")
        torch.cuda.current_stream(sx.device).synchronize()
        L.check(L.lib().oemgpu_fit_logistic_sparse_fold_res(context(sx.device.index), sx.handle, yd.data_ptr(), None if fd is None else fd.data_ptr(),
                                                            int(nfolds), int(leave_out), int(bool(standardize)), int(bool(intercept)),
                                                            int(irls_maxit), float(irls_tol), C.byref(a.c), *a.outputs(p + 1)))
        if fd is not None and int(leave_out) > 0:
            n = int(n - (fd == int(leave_out)).sum().item())
        return OemFitBinomial(_decorate(a, penalty, varnames, True, n, p, family="binomial"))
    colptr, rowidx, vals = _csc_arrays(x)
    L.check(L.lib().oemgpu_fit_logistic_sparse(n, p, colptr.ctypes.data, _iptr(rowidx), _dptr(vals), _dptr(yh), int(bool(standardize)),
                                               int(bool(intercept)), int(irls_maxit), float(irls_tol), C.byref(a.c), *a.outputs(p + 1)))
    return OemFitBinomial(_decorate(a, penalty, varnames, True, n, p, family="binomial"))


def logistic_stats():
    """oemgpu_last_logistic_stats of this thread, as a dict"""
    out = (C.c_double * 8)()
    L.check(L.lib().oemgpu_last_logistic_stats(out))
    keys = ["rows_ms", "gram_ms", "inner_ms", "irls_steps", "inner_iters", "row_passes", "grams", "wall_ms"]
    return dict(zip(keys, list(out)))


# ------------------------------------------------------------------------------------------ oem.xtx()
def oem_xtx(xtx, xty, family="gaussian", penalty=None, lambda_=(), nlambda=100, lambda_min_ratio=None, alpha=1.0,
            gamma=3.0, tau=0.5, groups=(), scale_factor=(), penalty_factor=None, group_weights=None, maxit=500,
            tol=1e-7, irls_maxit=100, irls_tol=1e-3, varnames=None, interrupt=None):
    """oem.xtx(): R/oem_xtx.R:109-360.  interrupt: a callable polled on the calling thread while the library waits for the GPU
    (the R shim's is R_CheckUserInterrupt, ref src/oem_xtx.cpp:160-163); True ends the call with OEMGPU_ERR_INTERRUPTED."""
    L.sync_switches()
    penalty = _match_penalty(penalty)
    if getattr(xtx, "ndim", 0) != 2:
        raise ValueError("xtx must be a matrix")
    if xtx.shape[0] != xtx.shape[1]:
        raise ValueError("xtx must be a square matrix equal to X'X. do NOT provide design matrix")
    p = xtx.shape[1]
    xlen = xty.shape[0] if hasattr(xty, "shape") else len(xty)
    if p != xlen:
        raise ValueError("xty must have length equal to the number of columns and rows of xtx. do NOT provide response vector")
    if p < 2:
        raise ValueError("xtx must have at least two columns")
    if family == "binomial":
        raise ValueError("binomial not implemented yet")
    a, varnames = _fit_options(p, p, penalty, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups, penalty_factor, group_weights,
                               maxit, tol, irls_maxit, irls_tol, varnames, False, groups_sentence=True,   # (no n: the ratio's default is 0.0001)
                               interrupt=interrupt)
    sf = np.asarray(scale_factor, dtype=np.float64).ravel()
    if sf.size > 0 and sf.size != p:
        raise ValueError("scale.factor must be same length as xty (nvars)")
    lib = L.lib()
    if _is_torch_cuda(xtx):
        import torch
        xp, _, _, ld, keep = _device_matrix(xtx)
        if ld != p:
            keep = xtx.t().contiguous(); xp = keep.data_ptr()
        yd = xty if _is_torch_cuda(xty) else torch.as_tensor(np.asarray(xty, dtype=np.float64), device=xtx.device)
        yd = yd.to(torch.float64).contiguous().reshape(-1)
        ctx = context(xtx.device.index)
        torch.cuda.current_stream(xtx.device).synchronize()
        L.check(lib.oemgpu_fit_xtx_dev(ctx, xp, yd.data_ptr(), p, _dptr(sf), C.byref(a.c), *a.outputs(p)))
        del keep
    else:
        xh = np.asfortranarray(xtx, dtype=np.float64)
        yh = np.ascontiguousarray(np.asarray(xty, dtype=np.float64).reshape(-1))
        L.check(lib.oemgpu_fit_xtx(_dptr(xh), _dptr(yh), p, _dptr(sf), C.byref(a.c), *a.outputs(p)))
    return _decorate(a, penalty, varnames, False, None, p)


# ------------------------------------------------------------------------------------------ big.oem()
def big_oem(x, y, family="gaussian", penalty=None, weights=(), lambda_=(), nlambda=100, lambda_min_ratio=None,
            alpha=1.0, gamma=3.0, tau=0.5, groups=(), penalty_factor=None, group_weights=None, standardize=True,
            intercept=True, maxit=500, tol=1e-7, irls_maxit=100, irls_tol=1e-3, compute_loss=False, gigs=4.0,
            hessian_type="full", varnames=None, ngpus=0, devices=None, upload_threads=0, interrupt=None):
    """big.oem(): R/big_oem.R:121-441.  x: a (host) matrix or a list of row shards (the big.matrix stand-in);
    y: a vector or the matching list of shards."""
    L.sync_switches()
    penalty = PENALTIES if penalty is None else _match_penalty(penalty)      # match.arg(several.ok=TRUE), no default narrowing
    shards = list(x) if isinstance(x, (list, tuple)) else [x]
    yshards = list(y) if isinstance(y, (list, tuple)) else [y]
    if family == "binomial":
        raise ValueError("binomial case not implemented yet")
    if any(getattr(s, "ndim", 0) != 2 for s in shards):
        raise ValueError("x must have at least two columns")
    p = shards[0].shape[1]
    n = sum(s.shape[0] for s in shards)
    if p < 2:
        raise ValueError("x must have at least two columns")
    if len(weights) > 0:
        raise ValueError("weights not implemented yet.")
    if len(yshards) != len(shards) or sum(len(v) for v in yshards) != n:
        raise ValueError("x and y lengths do not match")
    a, varnames = _fit_options(n, p, penalty, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups, penalty_factor, group_weights,
                               maxit, tol, irls_maxit, irls_tol, varnames, bool(intercept), groups_sentence=True, compute_loss=compute_loss,
                               ngpus=ngpus, devices=devices, upload_threads=upload_threads, interrupt=interrupt)
    xs = [np.asfortranarray(s, dtype=np.float64) for s in shards]
    ys = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in yshards]
    ns = (C.c_int64 * len(xs))(*[s.shape[0] for s in xs])
    xp = (L._dp * len(xs))(*[_dptr(s) for s in xs])
    yp = (L._dp * len(ys))(*[_dptr(v) for v in ys])
    L.check(L.lib().oemgpu_fit_big(xp, ns, len(xs), p, yp, int(bool(standardize)), int(bool(intercept)),
                                   C.byref(a.c), *a.outputs(p + 1)))
    return _decorate(a, penalty, varnames, True, n, p)



# ------------------------------------------------------------------------------------------ xval.oem()
def _getmin(lam, cvm, cvsd):
    """R/utils.R:3-26 (getmin)"""
    lmin_models, l1se_models, cv_models = [], [], []
    for m in range(len(cvm)):
        cvmin = np.min(cvm[m])
        idmin = cvm[m] <= cvmin
        lmin = np.max(lam[m][idmin])
        cv_models.append(np.min(cvm[m][idmin]))
        i0 = int(np.nonzero(lam[m] == lmin)[0][0])
        semin = (cvm[m] + cvsd[m])[i0]
        l1se_models.append(np.max(lam[m][cvm[m] < semin]))
        lmin_models.append(lmin)
    mmin = int(np.argmin(cv_models))
    return {"lambda.min": lmin_models[mmin], "model.min": mmin + 1, "lambda.1se": l1se_models[mmin],
            "lambda.min.models": np.array(lmin_models), "lambda.1se.models": np.array(l1se_models)}


_TYPE_MEASURES = ("mse", "deviance", "class", "auc", "mae")
_GAUSSIAN_NAMES = {"mse": "Mean-Squared Error", "mae": "Mean Absolute Error"}


def _check_type_measure(type_measure):
    """match.arg(type.measure) of xval.oem and cv.oem: "default" when none is given"""
    if type_measure is None:
        return "default"
    if type_measure not in _TYPE_MEASURES:
        raise ValueError("'arg' should be one of " + ", ".join("'%s'" % t for t in _TYPE_MEASURES))
    return type_measure


def _fold_ids(foldid, nfolds, n, rng):
    """(foldid, nfolds): the ids drawn with `rng` as sample(rep(seq(nfolds), length = n)), or the caller's and their largest"""
    if foldid is None:
        g = np.random.default_rng() if rng is None else rng
        foldid = g.permutation(np.resize(np.arange(1, int(nfolds) + 1), n))
    else:
        foldid = np.asarray(foldid).ravel()
        nfolds = int(foldid.max())
    if nfolds < 3:
        raise ValueError("nfolds must be bigger than 3; nfolds=10 recommended")
    return foldid, nfolds


def _gaussian_measure(type_measure):
    """"mse" or "mae" for a Gaussian model (R/oem_xval.R:488-497, R/cv_oem.R:357-363)"""
    if type_measure in ("default", "deviance"):
        return "mse"
    if type_measure not in ("mse", "mae"):
        warnings.warn("Only 'mse', 'deviance' or 'mae'  available for Gaussian models; 'mse' used")
        return "mse"
    return type_measure


def _ungrouped_if_small(n, nfolds, grouped):
    """`grouped`, or False where a fold holds fewer than three observations (R/cv_oem.R:405-411)"""
    if n / nfolds < 3 and grouped:
        warnings.warn("Option grouped=FALSE enforced in cv.glmnet, since < 3 observations per fold")
        return False
    return grouped


def xval_oem(x, y, nfolds=10, foldid=None, type_measure=None, ncores=-1, family="gaussian", penalty=None, weights=(),
             lambda_=(), nlambda=100, lambda_min_ratio=None, alpha=1.0, gamma=3.0, tau=0.5, groups=(), penalty_factor=None,
             group_weights=None, standardize=True, intercept=True, maxit=500, tol=1e-7, irls_maxit=100, irls_tol=1e-3,
             compute_loss=False, varnames=None, rng=None, ngpus=0, devices=None, upload_threads=0, interrupt=None):
    """xval.oem(): R/oem_xval.R:107-460 (gaussian; a dense x, or any scipy.sparse x -- oemgpu_xval_sparse, the same result as on
    x.toarray() without building it; no weights, ngpus or devices there).  foldid: values 1..nfolds; drawn with `rng` (a numpy Generator)
    as sample(rep(seq(nfolds), length = n)) when None.  ngpus / devices (host x only): the rows over several devices inside the
    library, as in oem().  A row-major float64 or float32 device tensor is gathered into fold order where it lies
    (oemgpu_xval_dense_rm_dev; _xval_rowmajor_in_place): the column-major call's result bit for bit, without its copies.
    An open SparseX runs oemgpu_xval_sparse_res on the resident columns (the scipy call's bits, nothing uploaded but y and foldid); a
    sparse torch tensor on a device is wrapped in one for the length of the call, one on the host becomes its scipy matrix."""
    x = _sparse_tensor_arg(x)
    if _is_torch_sparse(x):                                            # a sparse device tensor: a SparseX for the length of the call
        kw = {k: v for k, v in locals().items() if k not in ("x", "y")}
        with SparseX(x) as sx:
            return xval_oem(sx, y, **kw)
    L.sync_switches()
    if family not in ("gaussian", "binomial"):
        raise ValueError("'arg' should be one of 'gaussian', 'binomial'")
    penalty = _match_penalty(penalty)
    type_measure = _check_type_measure(type_measure)
    if family == "binomial":
        raise ValueError("binomial models not yet supported for xval, use cv.oem() instead")
    if getattr(x, "ndim", 0) != 2 and not isinstance(x, SparseX):
        raise ValueError("x must have at least two columns")
    n, p = x.shape
    if p >= n:
        raise ValueError("number of observations must be greater than the number of variables\n"
                         "             for xval, use cv.oem instead, or, preferably, use another package such as\n"
                         "             glmnet for the lasso, ncvreg for MCP/SCAD, or grpreg or gglasso for group lasso.")
    if p < 2:
        raise ValueError("x must have at least two columns")
    foldid, nfolds = _fold_ids(foldid, nfolds, n, rng)
    on_handle = isinstance(x, SparseX)                          # the resident columns: oemgpu_xval_sparse_res, nothing uploaded but y and foldid
    if on_handle:
        x.handle                                                 # (a closed SparseX raises here)
    sparse = _is_scipy_sparse(x) or on_handle                    # R/oem_xval.R:196-201 stops here; :500 names the routine served now
    if sparse and len(weights) > 0:
        raise ValueError("observation weights of xval.oem need a dense x: the weighted call scales a fold-ordered dense copy by "
                         "sqrt(w), which a sparse x never builds")
    if sparse and (int(ngpus) > 1 or devices is not None):
        raise ValueError("ngpus / devices of xval.oem need a dense x: the rows of a sparse x are not split over devices")
    ylen = y.shape[0] if hasattr(y, "shape") else len(y)
    if ylen != n or len(foldid) != n:
        raise ValueError("x and y lengths do not match")
    wh = None
    if len(weights) > 0:                                         # R/oem_xval.R:216-223
        if len(weights) != n:
            raise ValueError("length of weights not same as number of observations in x")
        wh = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    a, varnames = _fit_options(n, p, penalty, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups, penalty_factor, group_weights,
                               maxit, tol, irls_maxit, irls_tol, varnames, bool(intercept), groups_sentence=True, compute_loss=compute_loss,
                               ngpus=ngpus, devices=devices, upload_threads=upload_threads, interrupt=interrupt)
    type_measure = _gaussian_measure(type_measure)
    out = a.outputs(p + 1)
    cvm = np.zeros((a.npen, a.nl)); cvsd = np.zeros((a.npen, a.nl))
    fid = np.ascontiguousarray(foldid, dtype=np.int32)
    tm = 1 if type_measure == "mae" else 0
    lib = L.lib()
    if on_handle:
        import torch
        yd = _device_y(y, x.device).to(x.device)
        fd = torch.as_tensor(fid, device=x.device)
        torch.cuda.current_stream(x.device).synchronize()
        L.check(lib.oemgpu_xval_sparse_res(context(x.device.index), x.handle, yd.data_ptr(), fd.data_ptr(), int(nfolds), int(bool(standardize)),
                                           int(bool(intercept)), tm, C.byref(a.c), *out, _dptr(cvm), _dptr(cvsd)))
    elif sparse:
        colptr, rowidx, vals = _csc_arrays(x)
        yh = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        L.check(lib.oemgpu_xval_sparse(n, p, colptr.ctypes.data, rowidx.ctypes.data, vals.ctypes.data, yh.ctypes.data, fid.ctypes.data,
                                       int(nfolds), int(bool(standardize)), int(bool(intercept)), tm, C.byref(a.c), *out,
                                       _dptr(cvm), _dptr(cvsd)))
    elif _is_torch_cuda(x):
        import torch
        X = _DeviceX(x, _xval_rowmajor_in_place)                   # row-major: the rows go into fold order from where they lie, no copies
        yd = _device_y(y, x.device)
        fd = torch.as_tensor(fid, device=x.device)
        wd = None if wh is None else torch.as_tensor(wh, device=x.device)
        ctx = context(x.device.index)
        torch.cuda.current_stream(x.device).synchronize()
        X.call("xval_dense", ctx, yd.data_ptr(), None if wd is None else wd.data_ptr(), fd.data_ptr(), int(nfolds), int(bool(standardize)),
               int(bool(intercept)), tm, C.byref(a.c), *out, _dptr(cvm), _dptr(cvsd))
    else:
        xh = np.asfortranarray(x, dtype=np.float64)
        yh = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
        L.check(lib.oemgpu_xval_dense(_dptr(xh), n, p, _dptr(yh), None if wh is None else _dptr(wh), _iptr(fid), int(nfolds),
                                      int(bool(standardize)),
                                      int(bool(intercept)), tm, C.byref(a.c), *out, _dptr(cvm), _dptr(cvsd)))
    return _xval_result(a, penalty, varnames, n, p, cvm, cvsd, type_measure, fid)


def _xval_result(a, penalty, varnames, n, p, cvm, cvsd, type_measure, fid):
    """xval.oem's return value (R/oem_xval.R:430-460) from the outputs `a` holds (an _Args, or one response of many) and cvm / cvsd [npen, nl]"""
    res = _decorate(a, penalty, varnames, True, n, p)
    res["cvm"] = [cvm[k, :1].copy() if name == "ols" else cvm[k].copy() for k, name in enumerate(penalty)]
    res["cvsd"] = [cvsd[k, :1].copy() if name == "ols" else cvsd[k].copy() for k, name in enumerate(penalty)]
    res["name"] = _GAUSSIAN_NAMES[type_measure]
    res["foldid"] = fid
    res.update(_getmin([l[:len(c)] for l, c in zip(res["lambda"], res["cvm"])], res["cvm"], res["cvsd"]))
    res["cvup"] = [m + s for m, s in zip(res["cvm"], res["cvsd"])]
    res["cvlo"] = [m - s for m, s in zip(res["cvm"], res["cvsd"])]
    res["best.model"] = penalty[res["model.min"] - 1]
    return res


def xval_multi_plan(n, p, nfolds, m, npen=1, nl=100, num_cu=256):
    """oemgpu_selftest_xval_multi_plan (pure host arithmetic) as a dict"""
    out = (C.c_int64 * 20)()
    L.check(L.lib().oemgpu_selftest_xval_multi_plan(int(n), int(p), int(nfolds), int(m), int(npen), int(nl), int(num_cu), out))
    keys = ["nb", "solve_chunks", "engine", "route", "rows", "chunks_max", "passes", "block", "cv_nwg", "bytes_single", "bytes_col", "bytes_yp",
            "bytes_cfirst", "bytes_part", "bytes_comp", "bytes_tab", "bytes_cvpart", "bytes_cvout", "bytes", "cap"]
    return dict(zip(keys, [int(v) for v in out]))


def xval_multi_timings():
    """oemgpu_last_xval_multi_timings of this thread (ms; taken while oemgpu_set_timing is on) as a dict"""
    out = (C.c_double * 6)()
    L.check(L.lib().oemgpu_last_xval_multi_timings(out))
    return dict(zip(["fold_order", "fold_gram", "fold_xty", "compose", "paths", "cv_error"], list(out)))


def xval_multi_fold_moments(x, Y, foldid, nfolds):
    """Test infrastructure: oemgpu_selftest_xval_multi_fold_moments_dev -> the composed fold buffers, numpy [m, nfolds, p + 2, p + 2]
    indexed [r, k, i, j] = M[i, j] of fold k's rows of (x, Y[:, r]).  x as multi_moments takes it."""
    import torch
    if not _is_torch_cuda(x) or x.ndim != 2:
        raise ValueError("x must be a 2-D torch tensor on a GPU")
    n, p = x.shape
    if x.dtype == torch.float64 and x.stride(0) == 1 and x.stride(1) >= n:
        code, ld = -1, x.stride(1)
    else:
        code, ld = _rowmajor_dtype(x), x.stride(0)
        if code is None:
            raise ValueError("x must be column-major float64, or row-major float64 / float32 with unit column stride")
    Yd, rs, cs = _device_responses(Y, x.device)
    m = Yd.shape[1]
    fd = torch.as_tensor(np.ascontiguousarray(foldid, dtype=np.int32), device=x.device)
    out = torch.full((m, int(nfolds), p + 2, p + 2), float("nan"), dtype=torch.float64, device=x.device)
    ctx = context(x.device.index)
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_selftest_xval_multi_fold_moments_dev(ctx, x.data_ptr(), code, n, ld, p, Yd.data_ptr(), rs, cs, m, fd.data_ptr(),
                                                                int(nfolds), out.data_ptr()))
    return out.cpu().numpy().transpose(0, 1, 3, 2).copy()            # (the buffers are column-major)


def xval_oem_multi(x, Y, nfolds=10, foldid=None, type_measure=None, family="gaussian", penalty=None, weights=(), lambda_=(), nlambda=100,
                   lambda_min_ratio=None, alpha=1.0, gamma=3.0, tau=0.5, groups=(), penalty_factor=None, group_weights=None,
                   standardize=True, intercept=True, maxit=500, tol=1e-7, irls_maxit=100, irls_tol=1e-3, compute_loss=False, varnames=None,
                   rng=None, ngpus=0, devices=None, interrupt=None):
    """xval.oem for m responses on one resident x: [xval_oem(x, Y[:, r], foldid=foldid, ...) for r in range(m)] from one fold layout, one
    gather of x, one set of fold Gram passes, one X'Y pass over the fold-ordered rows, and the (K + 1) m paths in batched launches
    (include/oemgpu.h: oemgpu_xval_dense_multi_dev).  x: a dense torch device tensor, n x p with n > p >= 2, taken as
    xval_oem takes it (column-major float64 and row-major float64 / float32 read in place).  Y: n x m, taken as oem_multi takes it.
    foldid (values 1..nfolds; drawn once with `rng` when None) and a user lambda are shared by all responses.  xval_oem's other keyword
    arguments and checks.  Returns a list of m results with xval_oem's keys (predict_xval, plot_xval and summary_xval take them) and one
    more, `route`: 0 the response's K + 1 fits ran in a batched launch, 1 one launch (set) of their own, as xval_oem runs them."""
    host_or_sparse = ("xval_oem_multi() takes a dense torch tensor on a GPU: a host or sparse x is cross-validated one response at a "
                      "time with xval_oem()")
    if isinstance(x, SparseX) or _is_scipy_sparse(x) or _is_torch_sparse(x):
        raise ValueError(host_or_sparse)
    if family not in ("gaussian", "binomial"):
        raise ValueError("'arg' should be one of 'gaussian', 'binomial'")
    penalty = _match_penalty(penalty)
    type_measure = _check_type_measure(type_measure)
    if family == "binomial":
        raise ValueError("binomial models not yet supported for xval, use cv.oem() instead")
    if len(weights) > 0:
        raise ValueError("xval_oem_multi(): no observation weights; a weighted response is cross-validated with xval_oem(weights=)")
    if ngpus or devices is not None:
        raise ValueError("xval_oem_multi(): the rows of a resident x are not split over devices (ngpus / devices); xval_oem() splits a host x")
    if getattr(Y, "ndim", None) != 2:
        raise ValueError("Y must be a matrix of n rows and one column per response")
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must have at least two columns")
    n, p = x.shape
    m = int(Y.shape[1])
    if m < 1:
        raise ValueError("Y must have at least one column")
    if p >= n:
        raise ValueError("number of observations must be greater than the number of variables\n"
                         "             for xval, use cv.oem instead, or, preferably, use another package such as\n"
                         "             glmnet for the lasso, ncvreg for MCP/SCAD, or grpreg or gglasso for group lasso.")
    if p < 2:
        raise ValueError("x must have at least two columns")
    foldid, nfolds = _fold_ids(foldid, nfolds, n, rng)
    if Y.shape[0] != n or len(foldid) != n:
        raise ValueError("x and y lengths do not match")
    if not _is_torch_cuda(x):
        raise ValueError(host_or_sparse)
    a, varnames = _fit_options(n, p, penalty, lambda_, nlambda, lambda_min_ratio, alpha, gamma, tau, groups, penalty_factor, group_weights,
                               maxit, tol, irls_maxit, irls_tol, varnames, bool(intercept), groups_sentence=True, compute_loss=compute_loss,
                               interrupt=interrupt)
    type_measure = _gaussian_measure(type_measure)
    L.sync_switches()
    import torch
    X = _DeviceX(x, _xval_rowmajor_in_place)
    Yd, rs, cs = _device_responses(Y, x.device)
    fid = np.ascontiguousarray(foldid, dtype=np.int32)
    fd = torch.as_tensor(fid, device=x.device)
    out = _ManyOut(m, a, p + 1)
    cvm = np.zeros((m, a.npen, a.nl)); cvsd = np.zeros((m, a.npen, a.nl))
    route = np.zeros(m, dtype=np.int32)
    ctx = context(x.device.index)
    torch.cuda.current_stream(x.device).synchronize()
    X.call("xval_dense_multi", ctx, Yd.data_ptr(), rs, cs, m, fd.data_ptr(), int(nfolds), int(bool(standardize)), int(bool(intercept)),
           1 if type_measure == "mae" else 0, C.byref(a.c), *out.pointers(), _dptr(cvm), _dptr(cvsd), _iptr(route))
    fits = []
    for r in range(m):
        fit = _xval_result(out.one(r), penalty, varnames, n, p, cvm[r], cvsd[r], type_measure, fid)
        fit["route"] = int(route[r])
        fits.append(fit)
    return fits



def xval_cv_plan(n, p, nfolds, npen, nl, num_cu):
    """oemgpu_selftest_xval_cv_plan (needs no GPU): where the CV-error launch of xval.oem lands for this shape, as a dict -- lt (16-lambda
    tiles per pass), passes, form ("single" / "multi" / "chunk"), lds (dynamic bytes), chunks and last (coefficient chunks, rows of the
    last one) and nwg (workgroups per fold and penalty)."""
    out = (C.c_int64 * 7)()
    L.check(L.lib().oemgpu_selftest_xval_cv_plan(int(n), int(p), int(nfolds), int(npen), int(nl), int(num_cu), out))
    lt, passes, form, lds, chunks, last, nwg = list(out)
    return dict(lt=lt, passes=passes, form=("single", "multi", "chunk")[form], lds=lds, chunks=chunks, last=last, nwg=nwg)


_XVS_PLAN_KEYS = ("csc", "chunks_max", "chunks_per_range", "ranges_per_fold_max", "ranges_max", "tile_rows", "cv_nwg", "cv_waves", "cv_lblk",
                  "bytes", "align", "gram_lds", "worst_fold_ranges", "worst_ranges", "worst_rows", "worst_fold_end_chunk", "worst_fold_tiles", "worst_fold_tile_end")


def xval_sparse_plan(n, p, nnz, nfolds, npen, nl, num_cu):
    """oemgpu_selftest_xval_sparse_plan (needs no GPU): the plan of xval.oem on a sparse x as a dict -- the route (csc: True / False), the
    chunk and range bounds, the tile rows, the CV-error launch, the device bytes of the call, and the ranges for the folds
    (n - nfolds + 1, 1, 1, ...) as the call would cut them (include/oemgpu.h)."""
    out = (C.c_int64 * 18)()
    L.check(L.lib().oemgpu_selftest_xval_sparse_plan(int(n), int(p), int(nnz), int(nfolds), int(npen), int(nl), int(num_cu), out))
    d = dict(zip(_XVS_PLAN_KEYS, list(out)))
    d["csc"] = bool(d["csc"])
    return d


def xval_sparse_fold_moments(x, y, foldid, nfolds):
    """oemgpu_selftest_xval_sparse_fold_moments (test infrastructure): the nfolds moment buffers, nfolds x (p + 2) x (p + 2), of a
    scipy.sparse x in the fold order of xval.oem."""
    L.sync_switches()
    n, p = x.shape
    colptr, rowidx, vals = _csc_arrays(x)
    yh = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    fid = np.ascontiguousarray(foldid, dtype=np.int32)
    out = np.full((int(nfolds), p + 2, p + 2), np.nan)
    L.check(L.lib().oemgpu_selftest_xval_sparse_fold_moments(n, p, colptr.ctypes.data, rowidx.ctypes.data, vals.ctypes.data, yh.ctypes.data,
                                                             fid.ctypes.data, int(nfolds), _dptr(out)))
    return out


def xval_sparse_cv_error(x, y, foldid, nfolds, coef, type_measure="mse", triples=False):
    """oemgpu_selftest_xval_sparse_cv_error (test infrastructure): the CV-error phase of xval.oem on a scipy.sparse x and a coefficient
    table of the caller's, nfolds x npen x nl x (p + 1) with slot 0 the intercept.  Returns (cvm, cvsd), npen x nl each, or with
    triples=True the npen x nl x 3 array of (count, mean, M2)."""
    L.sync_switches()
    n, p = x.shape
    colptr, rowidx, vals = _csc_arrays(x)
    yh = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    fid = np.ascontiguousarray(foldid, dtype=np.int32)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    if coef.ndim != 4 or coef.shape[0] != int(nfolds) or coef.shape[3] != p + 1:
        raise ValueError("coef must be nfolds x npen x nl x (p + 1)")
    npen, nl = coef.shape[1:3]
    tm = {"mse": 0, "mae": 1}[type_measure]
    cvm = np.full((npen, nl), np.nan); cvsd = np.full((npen, nl), np.nan)
    tri = np.full((npen, nl, 3), np.nan) if triples else None
    L.check(L.lib().oemgpu_selftest_xval_sparse_cv_error(n, p, colptr.ctypes.data, rowidx.ctypes.data, vals.ctypes.data, yh.ctypes.data,
                                                         fid.ctypes.data, int(nfolds), _dptr(coef), npen, nl, tm, _dptr(cvm), _dptr(cvsd),
                                                         None if tri is None else _dptr(tri)))
    return tri if triples else (cvm, cvsd)


def xval_sparse_timings():
    """oemgpu_last_xval_sparse_timings: HIP-event times (ms) of the phases of this thread's last xval_oem call on a sparse x"""
    out = (C.c_double * 6)()
    L.check(L.lib().oemgpu_last_xval_sparse_timings(out))
    return dict(zip(("upload", "fold_order", "fold_moments", "compressed_rows", "fits", "cv_error"), list(out)))


def xval_cv_error(x, y, foldid, nfolds, coef, type_measure="mse", weights=None, triples=False, ctx=None):
    """oemgpu_selftest_xval_cv_error_dev (test infrastructure): the CV-error phase of xval.oem on a coefficient table of the caller's.
    x: a column-major float64 matrix on a GPU; y (float64), foldid (int32, 1 .. nfolds) and weights (float64 or None): device tensors;
    coef: nfolds x npen x nl x (p + 1) on the host, slot 0 the intercept.  Returns (cvm, cvsd), npen x nl each, or with triples=True the
    npen x nl x 3 array of (count, mean, M2)."""
    import torch
    xp, n, p, ld, keepalive = _device_matrix(x)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    if coef.ndim != 4 or coef.shape[0] != int(nfolds) or coef.shape[3] != p + 1:
        raise ValueError("coef must be nfolds x npen x nl x (p + 1)")
    npen, nl = coef.shape[1:3]
    tm = {"mse": 0, "mae": 1}[type_measure]
    cvm = np.full((npen, nl), np.nan); cvsd = np.full((npen, nl), np.nan)
    tri = np.full((npen, nl, 3), np.nan) if triples else None
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_selftest_xval_cv_error_dev(ctx if ctx is not None else context(x.device.index), xp, n, ld, p, y.data_ptr(),
                                                      None if weights is None else weights.data_ptr(), foldid.data_ptr(), int(nfolds),
                                                      _dptr(coef), npen, nl, tm, _dptr(cvm), _dptr(cvsd), None if tri is None else _dptr(tri)))
    del keepalive
    return tri if triples else (cvm, cvsd)


def cv_gaussian_score(x, y, foldid, nfolds, coef, ncol, type_measure="mse", predmat=False, ctx=None):
    """oemgpu_selftest_cv_score_dev (test infrastructure): the scoring entry of cv.oem(family = "gaussian"), oemgpu_cv_score_dev, after the
    fold layout alone, on a coefficient table of the caller's.  x: a float64 matrix on a GPU; y (float64), foldid (int32, 1 .. nfolds):
    device tensors; coef: nfolds x npen x nl x (p + 1) on the host; ncol: the valid leading columns per penalty.  Returns
    (triples: nfolds x npen x nl x 3 = (count, mean, M2) of every fold's errors; predmat: npen x nl x n on the host in the caller's row
    order, or None)."""
    import torch
    xp, n, p, ld, keepalive = _device_matrix(x)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    if coef.ndim != 4 or coef.shape[0] != int(nfolds) or coef.shape[3] != p + 1:
        raise ValueError("coef must be nfolds x npen x nl x (p + 1)")
    npen, nl = coef.shape[1:3]
    ncol = np.ascontiguousarray(ncol, dtype=np.int32)
    if ncol.shape != (npen,):
        raise ValueError("ncol must hold one count per penalty")
    tri = np.full((int(nfolds), npen, nl, 3), np.nan)
    pm = torch.empty((npen, nl, n), dtype=torch.float64, device=x.device) if predmat else None
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_selftest_cv_score_dev(ctx if ctx is not None else context(x.device.index), xp, n, ld, p, y.data_ptr(),
                                                 foldid.data_ptr(), int(nfolds), _dptr(coef), npen, nl, _iptr(ncol),
                                                 {"mse": 0, "mae": 1}[type_measure], _dptr(tri), pm.data_ptr() if predmat else None))
    del keepalive
    return tri, (pm.cpu().numpy() if predmat else None)


def cv_sparse_gaussian_score(x, y, foldid, nfolds, coef, ncol, type_measure="mse", predmat=False, ctx=None):
    """oemgpu_selftest_cv_sparse_score (test infrastructure): the scoring entry of cv.oem(family = "gaussian") on a SparseX,
    oemgpu_cv_sparse_score_res, after the fold layout and the compressed rows alone, on a coefficient table of the caller's.  x: a
    SparseX; y (float64), foldid (int32, 1 .. nfolds): device tensors; coef: nfolds x npen x nl x (p + 1) on the host; ncol: the valid
    leading columns per penalty.  Returns (triples: nfolds x npen x nl x 3 = (count, mean, M2) of every fold's errors; predmat: npen x nl x n
    on the host in the caller's row order, or None)."""
    import torch
    L.sync_switches()
    n, p = x.shape
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    if coef.ndim != 4 or coef.shape[0] != int(nfolds) or coef.shape[3] != p + 1:
        raise ValueError("coef must be nfolds x npen x nl x (p + 1)")
    npen, nl = coef.shape[1:3]
    ncol = np.ascontiguousarray(ncol, dtype=np.int32)
    if ncol.shape != (npen,):
        raise ValueError("ncol must hold one count per penalty")
    tri = np.full((int(nfolds), npen, nl, 3), np.nan)
    pm = torch.empty((npen, nl, n), dtype=torch.float64, device=x.device) if predmat else None
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_selftest_cv_sparse_score(ctx if ctx is not None else context(x.device.index), x.handle, y.data_ptr(),
                                                    foldid.data_ptr(), int(nfolds), _dptr(coef), npen, nl, _iptr(ncol),
                                                    {"mse": 0, "mae": 1}[type_measure], _dptr(tri), pm.data_ptr() if predmat else None))
    return tri, (pm.cpu().numpy() if predmat else None)


def cv_sparse_wide_score(x, y, foldid, nfolds, coef, ncol, type_measure="mse", predmat=False, ctx=None):
    """oemgpu_cv_sparse_wide_score_res on a coefficient table of the caller's: the arguments and results of cv_sparse_gaussian_score,
    from the SparseX's compressed rows in the caller's order (no fold layout, one fold's table on the device at a time)."""
    import torch
    L.sync_switches()
    n, p = x.shape
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    if coef.ndim != 4 or coef.shape[0] != int(nfolds) or coef.shape[3] != p + 1:
        raise ValueError("coef must be nfolds x npen x nl x (p + 1)")
    npen, nl = coef.shape[1:3]
    ncol = np.ascontiguousarray(ncol, dtype=np.int32)
    if ncol.shape != (npen,):
        raise ValueError("ncol must hold one count per penalty")
    tri = np.full((int(nfolds), npen, nl, 3), np.nan)
    pm = torch.empty((npen, nl, n), dtype=torch.float64, device=x.device) if predmat else None
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_cv_sparse_wide_score_res(ctx if ctx is not None else context(x.device.index), x.handle, y.data_ptr(),
                                                    foldid.data_ptr(), int(nfolds), _dptr(coef), npen, nl, _iptr(ncol),
                                                    {"mse": 0, "mae": 1}[type_measure], _dptr(tri), pm.data_ptr() if predmat else None))
    return tri, (pm.cpu().numpy() if predmat else None)


def sparse_wide_fold_fit(x, y, foldid, nfolds, leave_out, penalty=None, **kw):
    """oemgpu_fit_sparse_wide_fold_res: oem(x[foldid != leave_out], y[foldid != leave_out], intercept=False, ...) on a SparseX with
    n <= p where it lies (leave_out = 0: every row; foldid may then be None).  y (float64) and foldid (int32, 1 .. nfolds): device
    tensors.  Returns the fit as oem() decorates it, with nobs = the kept rows."""
    import torch
    penalty = _match_penalty(penalty)
    n, p = x.shape
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=".*optimized for n >> p.*")
        a, varnames, standardize, _ = oem(x, y, penalty=penalty, intercept=False, _args_only=True, **kw)
    kept = C.c_int64(0)
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_fit_sparse_wide_fold_res(context(x.device.index), x.handle, y.data_ptr(), None if foldid is None else foldid.data_ptr(),
                                                    int(nfolds), int(leave_out), int(standardize), C.byref(a.c), *a.outputs(p + 1), C.byref(kept)))
    return _decorate(a, penalty, varnames, True, int(kept.value), p)


SPW_PASSES = ("rows", "cols", "stats", "loss")


def sparse_wide_pass(x, kind, vec, row_lanes=0, col_lanes=0, foldid=None, nfolds=3, leave_out=0, standardize=False, scale=1.0, coef=None,
                     ctx=None):
    """oemgpu_selftest_sparse_wide_pass (test infrastructure): one pass of the sparse wide engine on a SparseX with n <= p after the
    fit's own setup, with the lanes per row / per column forced (0: the plan's).  kind: "rows" (vec: p doubles), "cols" (vec: n), "stats"
    or "loss" (vec = y: n; loss: coef = the tables, ncoef x (p + 1)); vec, foldid (int32) and coef: device tensors.  Every output is
    filled with NaN before the call.  Returns a dict: out (rows: n, cols: p, loss: ncoef; stats: xy), for stats also xy_std and stats
    (4 + 2 p + 2), info (row_lanes, col_lanes, long_rows, long_cols, longest_row, longest_col, kept, masked) and the two lists of long
    lines, sorted."""
    import torch
    n, p = x.shape
    pass_ = SPW_PASSES.index(kind)
    ncoef = 0 if coef is None else int(coef.shape[0])
    if coef is not None and (coef.dim() != 2 or coef.shape[1] != p + 1 or not coef.is_contiguous()):
        raise ValueError("coef must be a contiguous ncoef x (p + 1) tensor")
    if vec is not None and vec.numel() != (p if kind == "rows" else n):
        raise ValueError("vec has the wrong length for this pass")
    nan = lambda m: torch.full((m,), float("nan"), dtype=torch.float64, device=x.device)
    out = nan({"rows": n, "cols": p, "stats": p, "loss": max(ncoef, 1)}[kind])
    out2, st = (nan(p), nan(4 + 2 * p + 2)) if kind == "stats" else (None, None)
    info = (C.c_int64 * 8)()
    lrow, lcol = np.full(n, -1, np.int32), np.full(p, -1, np.int32)
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_selftest_sparse_wide_pass(ctx if ctx is not None else context(x.device.index), x.handle, pass_, int(row_lanes), int(col_lanes),
                                                     None if foldid is None else foldid.data_ptr(), int(nfolds), int(leave_out),
                                                     int(bool(standardize)), float(scale), None if vec is None else vec.data_ptr(),
                                                     None if coef is None else coef.data_ptr(), ncoef, out.data_ptr(),
                                                     None if out2 is None else out2.data_ptr(), None if st is None else st.data_ptr(), info,
                                                     lrow.ctypes.data, lcol.ctypes.data))
    keys = ("row_lanes", "col_lanes", "long_rows", "long_cols", "longest_row", "longest_col", "kept", "masked")
    r = {"out": out.cpu().numpy(), "info": dict(zip(keys, (int(v) for v in info)))}
    if kind == "stats":
        r["xy_std"], r["stats"] = out2.cpu().numpy(), st.cpu().numpy()
    r["long_row_list"], r["long_col_list"] = np.sort(lrow[:int(info[2])]), np.sort(lcol[:int(info[3])])
    return r


_CVS_PLAN_KEYS = ("csc", "nwg", "waves", "lblk", "part_bytes", "bytes", "xval_bytes", "fold_bytes", "own_bytes", "rows_max", "nl16", "align")


def cv_sparse_plan(n, p, nnz, nfolds, npen, nl, num_cu):
    """oemgpu_selftest_cv_sparse_plan (needs no GPU): the plan of cv.oem(family = "gaussian") on a SparseX as a dict -- the route of the
    fold moments (csc: True / False), the scoring launch (nwg workgroups, waves, lblk blocks of 64 lambdas), the bytes of its per-fold
    wave partials, the device bytes of the call and their three terms, the most rows of the fold-ordered layout (include/oemgpu.h)."""
    out = (C.c_int64 * 12)()
    L.check(L.lib().oemgpu_selftest_cv_sparse_plan(int(n), int(p), int(nnz), int(nfolds), int(npen), int(nl), int(num_cu), out))
    d = dict(zip(_CVS_PLAN_KEYS, list(out)))
    d["csc"] = bool(d["csc"])
    return d


# ------------------------------------------------------------------------------------------ cv.oem()
def logistic_cv_score(x, y, foldid, nfolds, coef, y_hi=None, predmat=False):
    """oemgpu_logistic_cv_score_dev: the error terms of cv.oemfit_binomial (R/cv_oem.R:315-327) over the held-out rows of a resident x.
    x: a column-major float64 matrix on a GPU, a row-major float64 / float32 one (oemgpu_logistic_cv_score_rm_dev reads it where it
    lies and returns the bits of the column-major entry on the same values), or a SparseX (oemgpu_logistic_cv_score_sparse_res: for finite tables the bits of the
    dense entry on the same matrix written out); y (float64) and foldid (int32, 1 .. nfolds): device tensors; coef: nfolds x ncol x
    (p + 1) on the host, the columns that score the rows of each fold.  Returns (sums: nfolds x ncol x 8 = [sum, sum of squares] of
    deviance, class, mse, mae; counts: the fold sizes; predmat: n x ncol on the host, or None).  predmat="device": the third item is
    the ncol x n device tensor the kernel wrote (column c = row c; rows of no fold stay NaN) and nothing is copied to the host."""
    import torch
    sparse = isinstance(x, SparseX)
    X = None if sparse else _DeviceX(x, _logistic_rowmajor_in_place)   # row-major float64 / float32: scored where it lies
    n, p = x.shape
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    if coef.ndim != 3 or coef.shape[0] != int(nfolds) or coef.shape[2] != p + 1:
        raise ValueError("coef must be nfolds x ncol x (p + 1)")
    ncol = coef.shape[1]
    sums = np.zeros((int(nfolds), ncol, 8))
    counts = np.zeros(int(nfolds), dtype=np.int64)
    pm = torch.full((ncol, n), float("nan"), dtype=torch.float64, device=x.device) if predmat else None
    if y_hi is None:
        y_hi = float(y.max().item())
    torch.cuda.current_stream(x.device).synchronize()
    if sparse:
        L.check(L.lib().oemgpu_logistic_cv_score_sparse_res(context(x.device.index), x.handle, y.data_ptr(), float(y_hi), foldid.data_ptr(),
                                                            int(nfolds), _dptr(coef), ncol, _dptr(sums),
                                                            counts.ctypes.data_as(C.POINTER(C.c_int64)), None if pm is None else pm.data_ptr()))
    else:
        X.call("logistic_cv_score", context(x.device.index), y.data_ptr(), float(y_hi), foldid.data_ptr(), int(nfolds), _dptr(coef), ncol,
               _dptr(sums), counts.ctypes.data_as(C.POINTER(C.c_int64)), None if pm is None else pm.data_ptr())
    if isinstance(predmat, str):
        if predmat != "device":
            raise ValueError("predmat must be True, False or \"device\"")
        return sums, counts, pm
    return sums, counts, None if pm is None else pm.t().cpu().numpy()


def logistic_cv_auc(predmat_dev, y, foldid, nfolds, y_hi=None):
    """oemgpu_logistic_cv_auc_dev: the integers behind the AUC of cv.oemfit_binomial (R/cv_oem.R:288-307 with auc.mat, R/utils.R:90-125)
    for every fold and column of a predmat that stays on the device.  predmat_dev: the ncol x n float64 device tensor of
    logistic_cv_score(..., predmat="device") (contiguous, column c of predmat = row c); y (float64) and foldid (int32, 1 .. nfolds):
    device tensors.  The rows of a fold are ordered by prob, ties in row order (numpy's stable argsort; NaN last), y2 = (y == y_hi).
    Returns (u: nfolds x ncol, n1: nfolds, n0: nfolds) as int64 arrays -- u[f, c] = over the rows with y2 = 1, the rows with y2 = 0 in
    front of each; n1, n0 = the fold's rows with y2 = 1 and the rest -- exact, the same on every call; _auc_from_counts turns them into
    the AUC."""
    import torch
    if predmat_dev.dim() != 2 or predmat_dev.dtype != torch.float64 or not predmat_dev.is_contiguous():
        raise ValueError("predmat_dev must be a contiguous ncol x n float64 device tensor")
    ncol, n = predmat_dev.shape
    if y.dtype != torch.float64 or foldid.dtype != torch.int32 or y.numel() != n or foldid.numel() != n:
        raise ValueError("y (float64) and foldid (int32) must have one entry per row of predmat")
    if y_hi is None:
        y_hi = float(y.max().item())
    u = np.zeros((int(nfolds), ncol), dtype=np.int64)
    n1 = np.zeros(int(nfolds), dtype=np.int64)
    n0 = np.zeros(int(nfolds), dtype=np.int64)
    i64 = C.POINTER(C.c_int64)
    torch.cuda.current_stream(predmat_dev.device).synchronize()
    L.check(L.lib().oemgpu_logistic_cv_auc_dev(context(predmat_dev.device.index), predmat_dev.data_ptr(), n, ncol, y.data_ptr(), float(y_hi),
                                               foldid.data_ptr(), int(nfolds), u.ctypes.data_as(i64), n1.ctypes.data_as(i64),
                                               n0.ctypes.data_as(i64)))
    return u, n1, n0


def cv_auc_plan(n, nfolds, ncol, num_cu, longest_fold):
    """oemgpu_selftest_cv_auc_plan (needs no GPU): where oemgpu_logistic_cv_auc_dev lands for this shape, as a dict -- tile (keys per
    tile of a pass), lmax (the longest segment sorted in LDS), cb and batches (columns per batch, batches), ws and lds (workspace and
    dynamic LDS bytes), form ("lds" / "hbm": the longest fold's), chunk and chunks (the counting sort by fold)."""
    out = (C.c_int64 * 9)()
    L.check(L.lib().oemgpu_selftest_cv_auc_plan(int(n), int(nfolds), int(ncol), int(num_cu), int(longest_fold), out))
    tile, lmax, cb, batches, ws, lds, hbm, chunk, chunks = list(out)
    return dict(tile=tile, lmax=lmax, cb=cb, batches=batches, ws=ws, lds=lds, form=("lds", "hbm")[hbm], chunk=chunk, chunks=chunks)


def _auc_from_counts(u, n1, n0):
    """u / (n1 n0) as auc.mat writes it (R/utils.R:120-124): through the logarithms; 0/0 and x/0 come out as NaN, as there."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.exp(np.log(u) - np.log(n1) - np.log(n0)))


def _auc_rows(y2, prob):
    """auc.mat with unit weights (R/utils.R:90-125): the rows in the order of prob -- ties in row order, where the reference draws runif
    (any order is one of its draws) -- and, over the rows with y2 = 1, the rows with y2 = 0 in front of each."""
    ys = y2[np.argsort(prob, kind="stable")]
    n1 = float(ys.sum())
    n0 = float(len(ys)) - n1
    u = float(np.sum(np.cumsum(1.0 - ys)[ys == 1]))
    return _auc_from_counts(u, n1, n0)


_BINOMIAL_NAMES = {"mse": "Mean-Squared Error", "mae": "Mean Absolute Error", "deviance": "Binomial Deviance", "auc": "AUC",
                   "class": "Misclassification Error"}


def _cv_oem_binomial(x, y, penalty, weights, lambda_, type_measure, nfolds, foldid, grouped, keep, rng, kw):
    """cv.oem() for family = "binomial": R/cv_oem.R:56-221 with cv.oemfit_binomial (:224-346).  x is on the device once; the full fit,
    the K fold fits (masked row passes over that x, one fold after another) and the scoring all read it there.  A dense x (numpy or
    a device tensor) stays a column-major device matrix -- except a row-major float64 / float32 device tensor, which stays as it is
    and is read in place (_logistic_rowmajor_in_place); a scipy.sparse x becomes one SparseX, which is closed on the way out."""
    for drop in ("accelerate", "ncores"):            # oem() arguments the binomial fit has no use for (no Nesterov step, no OpenMP)
        kw.pop(drop, None)
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must have at least two columns")
    n, p = x.shape
    if len(weights) > 0:                                               # R/oem.R:244
        raise L.OemgpuError(-4, "weights not implemented yet.")
    yh = np.asarray(y.cpu() if _is_torch_cuda(y) else y, dtype=np.float64).reshape(-1)
    if yh.shape[0] != n:
        raise ValueError("x and y lengths do not match")
    if len(np.unique(yh)) > 2:                                         # R/oem.R:250-252
        raise ValueError("y must be a binary outcome")
    import torch
    lam_arg = () if lambda_ is None else lambda_
    if _is_scipy_sparse(x) or _is_torch_sparse(x):
        with SparseX(x) as sx:                                         # the one upload (a device tensor: none), the one compressed-row build
            yd = torch.as_tensor(yh, device=sx.device)

            def fit(fd, nfolds, leave_out):                            # the full fit is leave_out = 0 on the same handle
                return oem_fit_logistic_sparse(sx, yh, penalty=penalty, lambda_=lam_arg, _fold=(sx, fd, max(int(nfolds), 3), leave_out, yd), **kw)
            return _cv_oem_binomial_on(fit, lambda fd, nfolds, coef, **k: logistic_cv_score(sx, yd, fd, nfolds, coef, **k), sx.device,
                                       n, p, yh, penalty, type_measure, nfolds, foldid, grouped, keep, rng, yd)
    if _is_torch_cuda(x):                                              # row-major float64 / float32: as it lies; else column-major, once
        xd = _DeviceX(x, _logistic_rowmajor_in_place).resident
    else:
        xd = torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64).T), device="cuda").t()     # the one upload
    yd = torch.as_tensor(yh, device=xd.device)

    def fit(fd, nfolds, leave_out):
        if leave_out == 0:
            return oem_fit_logistic_dense(xd, yh, penalty=penalty, lambda_=lam_arg, **kw)
        return oem_fit_logistic_dense(xd, yh, penalty=penalty, lambda_=lam_arg, _fold=(fd, nfolds, leave_out, yd), **kw)
    return _cv_oem_binomial_on(fit, lambda fd, nfolds, coef, **k: logistic_cv_score(xd, yd, fd, nfolds, coef, **k), xd.device,
                               n, p, yh, penalty, type_measure, nfolds, foldid, grouped, keep, rng, yd)


def _cv_oem_binomial_on(fit, score, device, n, p, yh, penalty, type_measure, nfolds, foldid, grouped, keep, rng, yd):
    """_cv_oem_binomial once x is resident.  fit(foldid_dev, nfolds, leave_out): the fit without fold leave_out (0: the full fit, made
    before the folds are drawn: foldid_dev is then None); score(foldid_dev, nfolds, coef, y_hi=, predmat=): logistic_cv_score on that x;
    yd: y on the device (the AUC reads it there)."""
    import torch
    fit0 = fit(None, 0, 0)
    nmodels = len(penalty)
    foldid, nfolds = _fold_ids(foldid, nfolds, n, rng)
    if len(foldid) != n:
        raise ValueError("x and y lengths do not match")
    fd = torch.as_tensor(np.ascontiguousarray(foldid, dtype=np.int32), device=device)
    outlist = [fit(fd, nfolds, i) for i in range(1, nfolds + 1)]
    # cv.oemfit_binomial
    if type_measure == "default":
        type_measure = "deviance"
    if n / nfolds < 10 and type_measure == "auc":
        warnings.warn("Too few (< 10) observations per fold for type.measure='auc' in cv.lognet; changed to type.measure='deviance'. "
                      "Alternatively, use smaller value for nfolds")
        type_measure = "deviance"
    grouped = _ungrouped_if_small(n, nfolds, grouped)
    lam = [np.asarray(l, dtype=np.float64) for l in fit0["lambda"]]
    nl = len(lam[0])
    which_lam = [lam[m] >= max(np.min(o["lambda"][m]) for o in outlist) for m in range(nmodels)]     # no extrapolation to smaller lambdas
    y_hi = float(yh.max())                                            # the second level of as.factor(y)
    term = {"deviance": 0, "class": 2, "mse": 4, "mae": 6}.get(type_measure)
    predlist, cvraw, w = [], [], []
    good = np.zeros((nfolds, nl))
    nlami = 0
    for m in range(nmodels):
        nlami = int(which_lam[m].sum())
        s = lam[m][which_lam[m]]
        coef = np.empty((nfolds, nlami, p + 1))
        for i, o in enumerate(outlist):                                # predict.oem's interpolation (R/methods.R:48-109), coefficients only
            left, right, frac = _lambda_interp(np.asarray(o["lambda"][m], dtype=np.float64), s)
            b = np.asarray(o["beta"][m])
            coef[i] = (b[:, left] * frac + b[:, right] * (1 - frac)).T
        sums, counts, pm = score(fd, nfolds, coef, y_hi=y_hi, predmat="device" if type_measure == "auc" else bool(keep))
        if type_measure == "auc":                                      # per fold and column, on the device (R/cv_oem.R:288-307)
            au, an1, an0 = logistic_cv_auc(pm, yd, fd, nfolds, y_hi=y_hi)
            pm = pm.t().cpu().numpy() if keep else None                # the host copy only for fit.preval
        if keep:
            full = np.full((n, nl), np.nan)
            full[:, :nlami] = pm
            predlist.append(full)
        wisum = counts.astype(np.float64)
        if type_measure == "auc":
            raw = np.full((nfolds, nl), np.nan)
            for i in range(nfolds):
                for j in range(nlami):
                    raw[i, j] = _auc_from_counts(float(au[i, j]), float(an1[i]), float(an0[i]))
            cvraw.append(raw); w.append(wisum)
        elif grouped:                                                  # cvcompute (R/utils.R:128-144): fold means, weighted by fold size
            raw = np.full((nfolds, nl), np.nan)
            with np.errstate(invalid="ignore", divide="ignore"):
                raw[:, :nlami] = sums[:, :, term] / wisum[:, None]
            cvraw.append(raw); w.append(wisum)
        else:
            cvraw.append((sums[:, :, term].sum(axis=0), sums[:, :, term + 1].sum(axis=0), nlami))
    good[:, :nlami] = 1                                               # nlams[i] = nlami of the LAST model (R/cv_oem.R:286), for every fold
    cvm, cvsd = [], []
    for m in range(nmodels):
        if type_measure == "auc" or grouped:
            Nm = good.sum(axis=0)
            ok = ~np.isnan(cvraw[m])
            wsum = (ok * w[m][:, None]).sum(axis=0)
            with np.errstate(invalid="ignore", divide="ignore"):
                cm = np.where(ok, cvraw[m] * w[m][:, None], 0.0).sum(axis=0) / wsum
                cs = np.sqrt(np.where(ok, (cvraw[m] - cm) ** 2 * w[m][:, None], 0.0).sum(axis=0) / wsum / (Nm - 1))
        else:                                                          # rows as they are: mean and mean squared deviation from the sums
            s1, s2, k = cvraw[m]
            cm, cs = np.full(nl, np.nan), np.full(nl, np.nan)
            cm[:k] = s1 / n
            with np.errstate(invalid="ignore", divide="ignore"):
                cs[:k] = np.sqrt(np.maximum((s2 - 2.0 * cm[:k] * s1 + n * cm[:k] ** 2) / n, 0.0) / (n - 1))
        cvm.append(cm); cvsd.append(cs)
    return _cv_result(fit0, penalty, lam, cvm, cvsd, _BINOMIAL_NAMES[type_measure], predlist if keep else None, foldid)


def cv_oem_logistic_multi(x, Y, penalty=None, lambda_=None, type_measure=None, nfolds=10, foldid=None, grouped=True, keep=False, rng=None, **kw):
    """[cv_oem(x, Y[:, r], family="binomial", foldid=f, ...) for r in range(m)] for the m binomial responses of Y on one resident x, with
    ONE foldid f for all of them (drawn once when not given) and ONE call that makes all m (K + 1) fits in lock-step
    (oem_fit_logistic_dense_multi_folds).  From the fits on it is cv_oem's own code (_cv_oem_binomial_on): the held-out
    rows of response r are scored by logistic_cv_score / logistic_cv_auc on the device column Y[:, r], once per response.  Every element
    has cv_oem's keys (predict_cv, plot_cv and summary_cv take it) and one more, "route" = "multi_folds".  x: a dense torch tensor on a
    GPU with p + intercept <= 1024; the keyword arguments are oem_fit_logistic_dense_multi's.  ValueErrors before a device is looked for:
    hessian_type="full", weights, a host or sparse x, ngpus / devices, p + intercept > 1024, len(lambda_) < 2, nfolds < 3."""
    penalty = _match_penalty(penalty)
    type_measure = _check_type_measure(type_measure)
    if lambda_ is not None and len(lambda_) < 2:
        raise ValueError("Need more than one value of lambda for cv.oem")
    for drop in ("accelerate", "ncores"):            # oem() arguments the binomial fit has no use for (no Nesterov step, no OpenMP)
        kw.pop(drop, None)
    if kw.pop("ngpus", 0) or kw.pop("devices", None) is not None:
        raise ValueError("cv_oem_logistic_multi() runs on the one device that holds x: ngpus / devices are not served")
    if len(kw.pop("weights", ())) > 0:
        raise ValueError("weights not implemented yet.")
    if kw.get("hessian_type", "upper.bound") == "full":
        raise ValueError("hessian_type='full' builds one Hessian per response and IRLS step: call cv_oem(family='binomial') for each column")
    if isinstance(x, SparseX) or _is_scipy_sparse(x) or _is_torch_sparse(x) or not _is_torch_cuda(x):
        raise ValueError("cv_oem_logistic_multi() takes a dense torch tensor on a GPU: a host or sparse x is cross-validated one response at a "
                         "time with cv_oem(family='binomial')")
    if getattr(x, "ndim", 0) != 2 or x.shape[1] < 2:
        raise ValueError("x must have at least two columns")
    if getattr(Y, "ndim", None) != 2:
        raise ValueError("Y must be a matrix of n rows and one column per response")
    n, p = x.shape
    if Y.shape[0] != n:
        raise ValueError("x and y lengths do not match")
    if p + int(bool(kw.get("intercept", True))) > 1024:
        raise ValueError("cv_oem_logistic_multi() serves p + intercept <= 1024: call cv_oem(family='binomial') for each column")
    if foldid is None:
        if int(nfolds) < 3:
            raise ValueError("nfolds must be bigger than 3; nfolds=10 recommended")
        foldid, _ = _fold_ids(None, nfolds, n, rng)
    else:
        foldid = np.asarray(foldid.cpu() if _is_torch_cuda(foldid) else foldid).ravel()
    import torch
    lam_arg = () if lambda_ is None else lambda_
    fits = oem_fit_logistic_dense_multi_folds(x, Y, foldid, penalty=penalty, lambda_=lam_arg, **kw)
    xd = _DeviceX(x, _logistic_rowmajor_in_place).resident
    Yd, _, _ = _device_responses(Y, xd.device)
    out = []
    for r, mine in enumerate(fits):
        yd = Yd[:, r].contiguous()
        yh = yd.cpu().numpy()
        res = _cv_oem_binomial_on(lambda fd, nf, leave_out, mine=mine: mine[leave_out],
                                  lambda fd, nf, coef, yd=yd, **k: logistic_cv_score(xd, yd, fd, nf, coef, **k), xd.device, n, p, yh, penalty,
                                  type_measure, nfolds, foldid, grouped, keep, rng, yd)
        res["route"] = "multi_folds"
        out.append(res)
    return out


def _cv_gaussian_resident(x, penalty, kw, foldid, nfolds):
    """Whether cv_oem(family = "gaussian") runs on the x where it is: a dense device tensor, no "ols", one device, and every fold fit in
    the Gram form (more kept rows than columns).  Anything else is the host loop."""
    if not _is_torch_cuda(x) or getattr(x, "is_sparse", False) or "ols" in penalty:
        return False
    if kw.get("ngpus") or kw.get("devices") is not None or kw.get("_entry_weights") is not None:
        return False
    n, p = x.shape
    if len(foldid) != n or not np.issubdtype(foldid.dtype, np.integer) or foldid.min() < 1 or not 2 <= nfolds <= 512:
        return False
    return bool(np.all(n - np.bincount(foldid, minlength=nfolds + 1)[1:] > p))


def _cv_gaussian_fold_fits(x, y, foldid, nfolds, penalty, lam_arg, kw):
    """The K calls oem(x[!which, ], y[!which], ...) of R/cv_oem.R:155-175 on the resident x: oemgpu_cv_fold_fits_dev, or
    oemgpu_cv_fold_fits_rm_dev on a row-major float64 / float32 tensor as it lies (the same fits bit for bit).  Returns the fold
    fits as oem() returns them and what the scoring needs (the context, the shapes, the fold sizes, the option block)."""
    import types
    import torch
    n, p = x.shape
    a, varnames, standardize, intercept = oem(x, y, penalty=penalty, lambda_=lam_arg, _args_only=True, **kw)
    X = _DeviceX(x, _xval_rowmajor_in_place)                       # row-major: the rows go into fold order from where they lie
    yd = _device_y(y, x.device)
    fd = torch.as_tensor(np.ascontiguousarray(foldid, dtype=np.int32), device=x.device)
    ctx = context(x.device.index)
    K, npen, nl = int(nfolds), a.npen, a.nl
    beta = np.zeros((K, npen, nl, p + 1))
    lam_out, loss = np.zeros((K, npen, nl)), np.zeros((K, npen, nl))
    niter = np.zeros((K, npen, nl), dtype=np.int32)
    d, fold_n = np.zeros(K), np.zeros(K, dtype=np.int64)
    torch.cuda.current_stream(x.device).synchronize()
    outs = (C.byref(a.c), _dptr(beta), _dptr(lam_out), _iptr(niter), _dptr(loss), _dptr(d), fold_n.ctypes.data_as(C.POINTER(C.c_int64)))
    X.call("cv_fold_fits", ctx, yd.data_ptr(), fd.data_ptr(), K, int(standardize), int(intercept), *outs)
    outlist = [_decorate(types.SimpleNamespace(beta=beta[i], lam_out=lam_out[i], niter=niter[i], loss=loss[i],
                                               d=types.SimpleNamespace(value=float(d[i]))), penalty, varnames, True, int(n - fold_n[i]), p)
               for i in range(K)]
    return outlist, {"ctx": ctx, "n": n, "p": p, "K": K, "args": a, "fold_n": fold_n, "device": x.device}


def _cv_gaussian_sparse_checks(x, y, penalty, kw):
    """What cv_oem refuses on a SparseX before any device work (the fold checks follow once foldid is known)"""
    if "ols" in penalty:
        raise ValueError("cv.oem on a SparseX: the \"ols\" penalty is not served")
    if kw.get("ngpus") or kw.get("devices") is not None:
        raise ValueError("cv.oem on a SparseX: the rows of a sparse x are not split over devices")
    x.handle                                                      # a closed SparseX raises here
    ylen = y.shape[0] if hasattr(y, "shape") else len(y)
    if ylen != x.shape[0]:
        raise ValueError("x and y lengths do not match")


def _cv_gaussian_sparse_fold_fits(x, y, foldid, nfolds, penalty, lam_arg, kw):
    """cv.oem's K + 1 calls of oem() on a dgCMatrix (R/cv_oem.R:105, 155-175 -> oem_fit_sparse) as ONE call on the resident SparseX:
    oemgpu_cv_sparse_fold_fits_res.  Returns the full fit and the fold fits as oem() on a scipy x returns them, and what the scoring needs."""
    import types
    import torch
    n, p = x.shape
    foldid = _cv_sparse_foldid(foldid, n, nfolds)
    kept = n - np.bincount(foldid, minlength=nfolds + 1)[1:]
    if np.any(kept <= p):
        i = int(np.argmax(kept <= p))
        raise ValueError(f"cv.oem on a SparseX: fold {i + 1} leaves {int(kept[i])} rows for {p} columns (a fit of p >= n is not served here)")
    a, varnames, standardize, intercept = oem(x, y, penalty=penalty, lambda_=lam_arg, _args_only=True, **kw)
    yd = _device_y(y, x.device).to(x.device)
    fd = torch.as_tensor(np.ascontiguousarray(foldid, dtype=np.int32), device=x.device)
    ctx = context(x.device.index)
    K, npen, nl = int(nfolds), a.npen, a.nl
    beta = np.zeros((K + 1, npen, nl, p + 1))
    lam_out, loss = np.zeros((K + 1, npen, nl)), np.zeros((K + 1, npen, nl))
    niter = np.zeros((K + 1, npen, nl), dtype=np.int32)
    d, fold_n = np.zeros(K + 1), np.zeros(K, dtype=np.int64)
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_cv_sparse_fold_fits_res(ctx, x.handle, yd.data_ptr(), fd.data_ptr(), K, int(standardize), int(intercept),
                                                   C.byref(a.c), _dptr(beta), _dptr(lam_out), _iptr(niter), _dptr(loss), _dptr(d),
                                                   fold_n.ctypes.data_as(C.POINTER(C.c_int64))))
    fits = [_decorate(types.SimpleNamespace(beta=beta[i], lam_out=lam_out[i], niter=niter[i], loss=loss[i],
                                            d=types.SimpleNamespace(value=float(d[i]))), penalty, varnames, True,
                      int(n - fold_n[i - 1]) if i else n, p) for i in range(K + 1)]
    return fits[0], fits[1:], {"ctx": ctx, "n": n, "p": p, "K": K, "args": a, "fold_n": fold_n, "device": x.device,
                               "score": L.lib().oemgpu_cv_sparse_score_res}


def _sparse_wide_intercept_refusal(n, p, a, standardize):
    """raises the library's own sentence for a sparse x with p >= n and an intercept: oemgpu_fit_sparse says it before it looks at the
    arrays or for a device, so the call carries the shape and the option block alone"""
    none = np.zeros(1, dtype=np.int64)
    L.check(L.lib().oemgpu_fit_sparse(n, p, none.ctypes.data, None, None, _dptr(np.zeros(1)), int(bool(standardize)), 1, C.byref(a.c),
                                      *a.outputs(1)))
    raise AssertionError("oemgpu_fit_sparse accepted a sparse x with p >= n and an intercept")


def _cv_gaussian_sparse_wide_fold_fits(x, y, foldid, nfolds, penalty, lam_arg, kw):
    """cv.oem's K + 1 calls of oem() (R/cv_oem.R:105, 155-175) on a resident SparseX with n <= p and no intercept: K + 1 calls of
    oemgpu_fit_sparse_wide_fold_res on the handle where it lies -- leave_out = 0 the full fit, leave_out = k the masked fold fit with
    the kept-row count wherever n enters.  Returns what _cv_gaussian_sparse_fold_fits returns; the scoring is
    oemgpu_cv_sparse_wide_score_res on the same handle, y and fold ids."""
    import torch
    n, p = x.shape
    foldid = _cv_sparse_foldid(foldid, n, nfolds)
    a, varnames, standardize, intercept = oem(x, y, penalty=penalty, lambda_=lam_arg, _args_only=True, **kw)
    if intercept:
        _sparse_wide_intercept_refusal(n, p, a, standardize)
    yd = _device_y(y, x.device).to(x.device)
    fd = torch.as_tensor(np.ascontiguousarray(foldid, dtype=np.int32), device=x.device)
    ctx = context(x.device.index)
    K = int(nfolds)
    fold_n = np.bincount(foldid, minlength=K + 1)[1:].astype(np.int64)
    lib = L.lib()
    fits = []
    torch.cuda.current_stream(x.device).synchronize()
    for k in range(K + 1):
        kept = C.c_int64(0)
        L.check(lib.oemgpu_fit_sparse_wide_fold_res(ctx, x.handle, yd.data_ptr(), fd.data_ptr(), K, k, int(standardize), C.byref(a.c),
                                                    *a.outputs(p + 1), C.byref(kept)))
        fits.append(_decorate(a, penalty, varnames, True, int(kept.value), p))

    def score(ctx_, n_, p_, K_, *rest):                            # (yd and fd live as long as the scoring may run)
        return lib.oemgpu_cv_sparse_wide_score_res(ctx_, x.handle, yd.data_ptr(), fd.data_ptr(), K_, *rest)
    return fits[0], fits[1:], {"ctx": ctx, "n": n, "p": p, "K": K, "args": a, "fold_n": fold_n, "device": x.device, "score": score}


def _cv_sparse_foldid(foldid, n, nfolds):
    """the fold ids of cv_oem on a SparseX, checked before any device work"""
    foldid = np.asarray(foldid)
    if len(foldid) != n or not np.issubdtype(foldid.dtype, np.integer) or foldid.min() < 1 or foldid.max() > nfolds:
        raise ValueError("foldid must hold one integer in 1..nfolds per row of x")
    if not 3 <= nfolds <= 512:
        raise ValueError("cv.oem on a SparseX: nfolds must be in 3..512")
    return foldid


def _cv_gaussian_table(outlist, lam, which_lam, p):
    """coef[K][npen][nl][p + 1] and ncol[npen]: every fold's coefficients at the full fit's lambdas that no fold has to extrapolate to
    (predict.oem's lambda.interp, R/methods.R:48-109), packed into the leading columns (R/cv_oem.R:364-391)."""
    K, nmodels, nl = len(outlist), len(lam), len(lam[0])
    coef = np.zeros((K, nmodels, nl, p + 1))
    ncol = np.array([int(wl.sum()) for wl in which_lam], dtype=np.int32)
    for m in range(nmodels):
        if ncol[m] > 0:
            for i, o in enumerate(outlist):
                coef[i, m, :ncol[m]] = predict(o, type="coefficients", s=lam[m][which_lam[m]], which_model=m).T
    return coef, ncol


def _cv_gaussian_score(dev, outlist, lam, which_lam, type_measure, keep):
    """The prediction loop and the per-fold statistics of cv.oemfit_gaussian (R/cv_oem.R:376-391) on the fold-ordered rows the fold fits
    left on the device: (triples[K][npen][nl][3] = (count, mean, M2) of every fold's errors, fit.preval per model or None)."""
    n, p, K = dev["n"], dev["p"], dev["K"]
    coef, ncol = _cv_gaussian_table(outlist, lam, which_lam, p)
    nmodels, nl = len(lam), len(lam[0])
    triples = np.zeros((K, nmodels, nl, 3))
    pm = None
    if keep:
        import torch
        pm = torch.empty((nmodels, nl, n), dtype=torch.float64, device=dev["device"])
        torch.cuda.current_stream(dev["device"]).synchronize()
    score = dev.get("score", L.lib().oemgpu_cv_score_dev)          # (a SparseX: oemgpu_cv_sparse_score_res, the same arguments)
    L.check(score(dev["ctx"], n, p, K, _dptr(coef), nmodels, nl, _iptr(ncol), int(type_measure == "mae"),
                  _dptr(triples), pm.data_ptr() if keep else None))
    return triples, ([np.ascontiguousarray(a.T) for a in pm.cpu().numpy()] if keep else None)


def _cv_gaussian_triple_stats(dev, triples, nlams, grouped):
    """(cvm, cvsd) per model from the per-fold (count, mean, M2).  grouped: cvcompute's fold means (NaN where a fold has no error),
    weighted by fold size, N from the valid columns (R/utils.R:128-144).  Not grouped: the K fold sets of a column are one set of rows, and
    oemgpu_xval_merge's sd of the mean is cvcompute's for rows with unit weights (R/cv_oem.R:405-411); NaN where no row has an error."""
    K, nmodels, nl = triples.shape[:3]
    if grouped:
        good = np.zeros((K, nl))
        for i in range(K):
            good[i, :nlams[i]] = 1
        return _cv_weighted_stats([triples[:, m, :, 1].copy() for m in range(nmodels)], [dev["fold_n"].astype(np.float64)] * nmodels,
                                  [good.sum(axis=0)] * nmodels)
    cvm, cvsd = np.zeros((nmodels, nl)), np.zeros((nmodels, nl))
    L.check(L.lib().oemgpu_xval_merge(_dptr(np.ascontiguousarray(triples)), K, C.byref(dev["args"].c), _dptr(cvm), _dptr(cvsd)))
    for m in range(nmodels):
        none = triples[:, m, :, 0].sum(axis=0) == 0
        cvm[m, none] = np.nan; cvsd[m, none] = np.nan
    return list(cvm), list(cvsd)


def _cv_gaussian_host_fits(x, y, foldid, nfolds, penalty, lam_arg, kw, parallel):
    """The host loop's fold fits: x and y on the host, K gathers of the kept rows, K calls of oem().  (fold fits, x, y)"""
    xh = np.asarray(x.cpu().numpy() if _is_torch_cuda(x) else x, dtype=np.float64)
    yh = np.asarray(y.cpu().numpy() if _is_torch_cuda(y) else y, dtype=np.float64).reshape(-1)

    def fold_fit(i):
        keep_rows = foldid != i
        return oem(np.asfortranarray(xh[keep_rows]), yh[keep_rows], penalty=penalty, lambda_=lam_arg, **kw)
    # the p > n warning was given once, by the full fit: only THAT message is silenced for the fold fits, and the filter list is
    # touched by the calling thread alone, around the whole block (catch_warnings is process-global state: not for worker threads)
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message=".*optimized for n >> p.*")
        if parallel:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(int(nfolds), 3 if parallel is True else int(parallel))) as ex:
                outlist = list(ex.map(fold_fit, range(1, nfolds + 1)))
        else:
            outlist = [fold_fit(i) for i in range(1, nfolds + 1)]
    return outlist, xh, yh


def _cv_gaussian_host_stats(predlist, yh, foldid, nfolds, nlams, type_measure, grouped):
    """(cvm, cvsd) per model from the host loop's prediction matrices (R/cv_oem.R:392-423)"""
    n, nmodels = len(yh), len(predlist)
    cvraw = [(yh[:, None] - pm) ** 2 if type_measure == "mse" else np.abs(yh[:, None] - pm) for pm in predlist]
    w = [np.ones(n) for _ in range(nmodels)]
    N = [n - np.isnan(pm).sum(axis=0) for pm in predlist]
    if grouped:                                                   # cvcompute: fold means, weighted by fold size
        wisum = np.array([np.sum(foldid == i) for i in range(1, nfolds + 1)], dtype=np.float64)
        for m in range(nmodels):
            out = np.full((nfolds, cvraw[m].shape[1]), np.nan)
            good = np.zeros_like(out)
            for i in range(nfolds):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    out[i] = np.nanmean(cvraw[m][foldid == i + 1], axis=0)
                good[i, :nlams[i]] = 1
            cvraw[m], w[m], N[m] = out, wisum, good.sum(axis=0)
    return _cv_weighted_stats(cvraw, w, N)


def _cv_weighted_stats(cvraw, w, N):
    """cvm = the weighted mean of every column over its entries that are not NaN, cvsd = sqrt(the weighted mean squared deviation / (N - 1))
    (R/cv_oem.R:412-416), per model"""
    def wmean(a, wt):
        ok = ~np.isnan(a)
        return np.array([np.sum(a[ok[:, j], j] * wt[ok[:, j]]) / np.sum(wt[ok[:, j]]) if ok[:, j].any() else np.nan
                         for j in range(a.shape[1])])
    cvm = [wmean(r, wt) for r, wt in zip(cvraw, w)]
    with np.errstate(invalid="ignore", divide="ignore"):
        cvsd = [np.sqrt(wmean((r - c) ** 2, wt) / (nn - 1)) for r, c, wt, nn in zip(cvraw, cvm, w, N)]
    return cvm, cvsd


def _cv_result(fit0, penalty, lam, cvm, cvsd, name, predlist=None, foldid=None):
    """cv.oem's return value (R/cv_oem.R:190-221) from the full fit, its lambdas and cvm / cvsd per model: the columns where any
    model's cvsd is NaN leave cvm, cvsd, nzero and lambda; `name` is the measure's ("AUC" is the one that getmin maximises);
    predlist (keep=TRUE) goes in as fit.preval, with foldid"""
    nz = [np.array([0 if v is None else len(v) for v in predict(fit0, type="nonzero", which_model=m)]) for m in range(len(penalty))]
    nas = np.zeros(len(lam[0]), dtype=bool)
    for c in cvsd:
        nas |= np.isnan(c)
    if nas.any():
        cvm = [c[~nas] for c in cvm]; cvsd = [c[~nas] for c in cvsd]
        nz = [c[~nas] for c in nz]; lam = [l[~nas] for l in lam]
    res = OemFit()
    res.update({"lambda": lam, "cvm": cvm, "cvsd": cvsd, "cvup": [a + b for a, b in zip(cvm, cvsd)],
                "cvlo": [a - b for a, b in zip(cvm, cvsd)], "nzero": nz, "name": name, "oem.fit": fit0})
    if predlist is not None:
        res["fit.preval"] = predlist; res["foldid"] = foldid
    res.update(_getmin(lam, [-c for c in cvm] if name == "AUC" else cvm, cvsd))
    res["best.model"] = penalty[res["model.min"] - 1]
    res["penalty"] = list(penalty)
    return res


def cv_oem(x, y, penalty=None, weights=(), lambda_=None, type_measure=None, nfolds=10, foldid=None, grouped=True, keep=False,
           rng=None, parallel=False, family="gaussian", **kw):
    """cv.oem(): R/cv_oem.R:56-221 with cv.oemfit_gaussian (:349-423) and cvcompute (R/utils.R:128-144): K + 1 calls of oem(),
    every fold on its own lambda sequence, errors interpolated onto the full fit's lambdas.
    A dense x that is a device tensor stays there (no "ols", every fold keeps more rows than columns; `parallel` is accepted and ignored):
    the rows go into fold order once, fold ff's fit is solved from the sum of the other folds' moment buffers -- oem()'s own
    standardisation, lambda grid and shift rule on the kept rows, oemgpu_cv_fold_fits_dev -- the folds' coefficients are interpolated
    here (predict's lambda.interp) and the held-out rows are scored where they lie (oemgpu_cv_score_dev: per-fold count, mean and M2;
    fit.preval in the caller's row order only with keep=True).  Any other x takes the host loop: K gathers of the kept rows, K calls of
    oem(), predictions and errors in numpy.  Both routes share everything from cvcompute on.
    family = "binomial" (cv.oemfit_binomial, :224-346; dense x): x goes to the device once (a numpy x is uploaded, a device tensor is used as it
    is); the full fit, the fold fits -- row passes over that x which leave the fold's rows out, oemgpu_fit_logistic_dense_fold_dev -- and
    the scoring of the held-out rows (oemgpu_logistic_cv_score_dev) read it there.  type_measure: "deviance" (default), "class", "mse",
    "mae" or "auc" (on the device, from the held-out probabilities where the scoring wrote them: oemgpu_logistic_cv_auc_dev, a stable
    sort per fold and column, ties in row order; only keep=True copies them to the host).  `parallel` is accepted and the folds still run
    one after another.  The options are those of oem_fit_logistic_dense; the result has the keys below with an OemFitBinomial `oem.fit`.
    family = "binomial" with a scipy.sparse x (R/cv_oem.R:129-175 on a dgCMatrix, which reaches oem_fit_logistic_sparse): one SparseX holds
    the compressed columns and their compressed-row copy on the device; the full fit (leave_out = 0), the fold fits (masked passes,
    oemgpu_fit_logistic_sparse_fold_res) and the scoring (oemgpu_logistic_cv_score_sparse_res) read it there.  The options are those of
    oem_fit_logistic_sparse (hessian_type is checked and ignored; an intercept needs standardize).
    family = "gaussian" on a sparse x (R/cv_oem.R:129-175 on a dgCMatrix, which reaches oem_fit_sparse) enters where the dense route does,
    on an x that is already resident: an oem_amd.SparseX.  cv.oem's K + 1 calls of oem() are ONE call, oemgpu_cv_sparse_fold_fits_res: the
    handle's columns go into fold order, the K fold moment buffers come from one pass over the non-zeros, and the full fit (`oem.fit`,
    wrapped as oem() on a scipy x wraps its result) and fold ff's fit are oemSparse's solve -- no centring, intval, the kept-row count
    wherever n enters -- on the sum of all buffers / of all but ff.  From there on it is the resident dense route's code: the folds'
    coefficients interpolated here, the held-out rows scored from the fold-ordered compressed rows (oemgpu_cv_sparse_score_res), fit.preval
    and foldid with keep=True; y may be numpy or a device tensor, `parallel` is accepted and ignored.  ValueErrors before any device work:
    "ols" among the penalties, weights, ngpus / devices, a closed SparseX, len(y) != n, nfolds < 3, a fold id outside 1..nfolds and a fold
    that keeps no more rows than columns (named: there is no host loop for a sparse x).  A scipy matrix itself with family = "gaussian"
    stays a ValueError.
    A SparseX with n <= p (and intercept=False: with an intercept the library's refusal of a sparse x with p >= n is raised) takes the
    wide form of all of it: the full fit and the K fold fits are K + 1 calls of oemgpu_fit_sparse_wide_fold_res on the handle where it
    lies (leave_out = 0, then 1..K: masked passes over the non-zeros, the kept-row count wherever n enters), the held-out rows are scored
    from the handle's compressed rows in the caller's order (oemgpu_cv_sparse_wide_score_res, one fold's table on the device at a time);
    the same refusals otherwise.
    parallel (R/cv_oem.R:32, 129-150: the folds through foreach): the fold fits from a few host threads at once.  On one GPU that
    pays where a fit leaves most of the chip idle: the path kernels of n >> p fits (one CU each) overlap with other folds' moment
    kernels, and p >= n fits on the cooperating-workgroup engine (a quarter of the CUs each) run side by side -- they queue for CU
    slots by themselves.  Same results as the sequential loop.  (Measured, six folds: 300 x 1500 136 -> 117 ms; 5000 x 40 8 -> 17 ms --
    fits of a millisecond lose more to the thread hand-over than the overlap gains: the default stays sequential, as in R.)"""
    if family not in ("gaussian", "binomial"):
        raise ValueError("'arg' should be one of 'gaussian', 'binomial'")
    penalty = _match_penalty(penalty)
    type_measure = _check_type_measure(type_measure)
    if lambda_ is not None and len(lambda_) < 2:
        raise ValueError("Need more than one value of lambda for cv.oem")
    x = _sparse_tensor_arg(x)
    if family == "binomial":
        return _cv_oem_binomial(x, y, penalty, weights, lambda_, type_measure, nfolds, foldid, grouped, keep, rng, kw)
    if len(weights) > 0:
        raise ValueError("weights not implemented yet.")
    if _is_torch_sparse(x):                                       # a sparse device tensor: a SparseX for the length of the call
        with SparseX(x) as sx:
            return cv_oem(sx, y, penalty=penalty, lambda_=lambda_, type_measure=None if type_measure == "default" else type_measure, nfolds=nfolds, foldid=foldid, grouped=grouped,
                          keep=keep, rng=rng, parallel=parallel, family=family, **kw)
    if _is_scipy_sparse(x):
        raise ValueError("cv.oem on a sparse x is served for family = \"binomial\" only (family = \"gaussian\" runs on a resident "
                         "oem_amd.SparseX(x), not on the scipy matrix)")
    on_sparse = isinstance(x, SparseX)
    if on_sparse:
        _cv_gaussian_sparse_checks(x, y, penalty, kw)
    elif getattr(x, "ndim", 0) != 2:
        raise ValueError("x must have at least two columns")
    n = x.shape[0]
    lam_arg = () if lambda_ is None else lambda_
    if not on_sparse:
        fit0 = oem(x, y, penalty=penalty, lambda_=lam_arg, **kw)
    foldid, nfolds = _fold_ids(foldid, nfolds, n, rng)
    resident = on_sparse or _cv_gaussian_resident(x, penalty, kw, foldid, nfolds)
    if on_sparse and x.shape[0] <= x.shape[1]:                    # n <= p: the full fit and the K masked fold fits over the handle's non-zeros
        fit0, outlist, dev = _cv_gaussian_sparse_wide_fold_fits(x, y, foldid, nfolds, penalty, lam_arg, kw)
    elif on_sparse:                                               # the full fit and the K fold fits from the fold moments of the resident columns
        fit0, outlist, dev = _cv_gaussian_sparse_fold_fits(x, y, foldid, nfolds, penalty, lam_arg, kw)
    elif resident:                                                # x stays where it is: fold moments, K solves (oemgpu_cv_fold_fits_dev)
        outlist, dev = _cv_gaussian_fold_fits(x, y, foldid, nfolds, penalty, lam_arg, kw)
    else:
        outlist, xh, yh = _cv_gaussian_host_fits(x, y, foldid, nfolds, penalty, lam_arg, kw, parallel)
    # cv.oemfit_gaussian
    type_measure = _gaussian_measure(type_measure)
    lam = [np.asarray(l, dtype=np.float64) for l in fit0["lambda"]]
    nmodels = len(penalty)
    which_lam = [lam[m] >= max(np.min(o["lambda"][m]) for o in outlist) for m in range(nmodels)]     # no extrapolation to smaller lambdas
    nlams = np.full(nfolds, int(which_lam[-1].sum()))             # nlami of the LAST model, for every fold (R/cv_oem.R:386-389)
    if resident:                                                  # interpolated tables up, per-fold (count, mean, M2) down (oemgpu_cv_score_dev)
        triples, predlist = _cv_gaussian_score(dev, outlist, lam, which_lam, type_measure, keep)
    else:
        predlist = [np.full((n, len(lam[0])), np.nan) for _ in range(nmodels)]
        for i in range(1, nfolds + 1):
            rows = foldid == i
            for m in range(nmodels):
                preds = predict(outlist[i - 1], xh[rows], s=lam[m][which_lam[m]], which_model=m)
                predlist[m][rows, :int(which_lam[m].sum())] = preds
    grouped = _ungrouped_if_small(n, nfolds, grouped)
    if resident:
        cvm, cvsd = _cv_gaussian_triple_stats(dev, triples, nlams, grouped)
    else:
        cvm, cvsd = _cv_gaussian_host_stats(predlist, yh, foldid, nfolds, nlams, type_measure, grouped)
    return _cv_result(fit0, penalty, lam, cvm, cvsd, _GAUSSIAN_NAMES[type_measure], predlist if keep else None, foldid)


def _cv_weighted_stats_many(cvraw, w, N):
    """_cv_weighted_stats for many tables at once, no loop over the columns: cvraw[..., K, nl] (NaN = no entry), w[K], N broadcast
    against [..., nl] -> (cvm, cvsd)[..., nl], the same values (a column without an entry: NaN)."""
    cvraw = np.asarray(cvraw, dtype=np.float64)
    wt = np.asarray(w, dtype=np.float64)[:, None]

    def wmean(a):
        ok = ~np.isnan(a)
        den = np.where(ok, wt, 0.0).sum(axis=-2)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(den > 0, np.where(ok, a * wt, 0.0).sum(axis=-2) / den, np.nan)
    cvm = wmean(cvraw)
    with np.errstate(invalid="ignore", divide="ignore"):
        cvsd = np.sqrt(wmean((cvraw - cvm[..., None, :]) ** 2) / (np.asarray(N, dtype=np.float64) - 1))
    return cvm, cvsd


def _cv_gaussian_triple_stats_many(fold_n, triples, ncol_last, grouped):
    """_cv_gaussian_triple_stats for R responses at once: triples[R, K, npen, nl, 3], ncol_last[R] (the valid columns of every response's
    LAST model: the nlams rule of R/cv_oem.R:386-389) -> (cvm, cvsd)[R, npen, nl], the same values.  Not grouped: oemgpu_xval_merge's
    sequential Chan update over the folds, one numpy step per fold."""
    triples = np.asarray(triples, dtype=np.float64)
    R, K, nmodels, nl = triples.shape[:4]
    if grouped:
        N = np.where(np.arange(nl)[None, :] < np.asarray(ncol_last).reshape(R, 1), float(K), 0.0)       # good.sum(axis=0)
        return _cv_weighted_stats_many(triples[..., 1].transpose(0, 2, 1, 3), np.asarray(fold_n, dtype=np.float64), N[:, None, :])
    na, ma, qa = (np.zeros((R, nmodels, nl)) for _ in range(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(K):
            nb, mb, qb = triples[:, s, :, :, 0], triples[:, s, :, :, 1], triples[:, s, :, :, 2]
            some, first = nb > 0.0, na <= 0.0
            nn, dl = na + nb, mb - ma
            m2 = ma + dl * (nb / nn)
            q2 = qa + (qb + dl * dl * (na * nb / nn))
            ma = np.where(some, np.where(first, mb, m2), ma)
            qa = np.where(some, np.where(first, qb, q2), qa)
            na = np.where(some, np.where(first, nb, nn), na)
        cvm = ma.copy()
        cvsd = np.where(na > 1.0, np.sqrt(np.maximum(qa, 0.0) / (na - 1.0)) / np.sqrt(na), 0.0)
    none = triples[..., 0].sum(axis=1) == 0
    cvm[none] = np.nan; cvsd[none] = np.nan
    return cvm, cvsd


def cv_multi_plan(n, p, nfolds, m, npen=1, nl=100, num_cu=256, keep=False, nb_limit=0):
    """oemgpu_selftest_cv_multi_plan (pure host arithmetic) as a dict: xval_multi_plan's keys (the solve plan read at q = p) and the
    regions cv_oem_multi adds"""
    out = (C.c_int64 * 27)()
    L.check(L.lib().oemgpu_selftest_cv_multi_plan(int(n), int(p), int(nfolds), int(m), int(npen), int(nl), int(num_cu), int(bool(keep)), int(nb_limit), out))
    keys = ["nb", "solve_chunks", "engine", "route", "rows", "chunks_max", "passes", "block", "cv_nwg", "bytes_single", "bytes_col", "bytes_yp",
            "bytes_cfirst", "bytes_part", "bytes_comp", "bytes_tab", "bytes_cvpart", "bytes_cvout", "bytes_xval", "cap", "bytes_raw", "bytes_idx",
            "bytes_ncol", "bytes_inv", "bytes_pred", "bytes_tri", "bytes"]
    return dict(zip(keys, [int(v) for v in out]))


def cv_multi_nb_limit(nb_limit):
    """Test infrastructure: oemgpu_selftest_cv_multi_nb_limit -- this thread's cv_oem_multi calls take at most nb_limit responses per
    chunk from now on (0: no limit)"""
    L.check(L.lib().oemgpu_selftest_cv_multi_nb_limit(int(nb_limit)))


def cv_multi_timings():
    """oemgpu_last_cv_multi_timings of this thread (ms; taken while oemgpu_set_timing is on) as a dict"""
    out = (C.c_double * 7)()
    L.check(L.lib().oemgpu_last_cv_multi_timings(out))
    return dict(zip(["fold_order", "fold_gram", "fold_xty", "compose", "paths", "interp", "score"], list(out)))


def cv_multi_interp_table(lam_full, lam_fold):
    """oemgpu_selftest_cv_interp (needs no GPU): lam_full[npen, nl], lam_fold[K, npen, nl] -> (left, right, frac)[K, npen, nl], ncol[npen]"""
    lam_full = np.ascontiguousarray(lam_full, dtype=np.float64)
    lam_fold = np.ascontiguousarray(lam_fold, dtype=np.float64)
    K, npen, nl = lam_fold.shape
    if lam_full.shape != (npen, nl):
        raise ValueError("lam_full must be [npen, nl] and lam_fold [K, npen, nl]")
    left, right = np.zeros((K, npen, nl), dtype=np.int32), np.zeros((K, npen, nl), dtype=np.int32)
    frac, ncol = np.zeros((K, npen, nl)), np.zeros(npen, dtype=np.int32)
    L.check(L.lib().oemgpu_selftest_cv_interp(K, npen, nl, _dptr(lam_full), _dptr(lam_fold), _iptr(left), _iptr(right), _dptr(frac), _iptr(ncol)))
    return left, right, frac, ncol


def cv_multi_score(x, Y, foldid, nfolds, coef, ncol, type_measure="mse", nb=1, interp=None, predmat=None, ctx=None):
    """Test infrastructure: oemgpu_selftest_cv_score_multi_dev.  x: a column-major float64 device tensor; coef[m, K, npen, nl, p + 1] and
    ncol[m, npen] on the host; interp = (left, right, frac)[m, K, npen, nl] sends coef through the interpolation kernel first; predmat:
    None or a float64 device tensor of m npen nl n elements, written in place.  -> (triples[m, K, npen, nl, 3], the table the
    interpolation wrote or None)"""
    import torch
    ptr, n, p, ld, keepalive = _device_matrix(x)
    Yd, rs, cs = _device_responses(Y, x.device)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    m, K, npen, nl = coef.shape[:4]
    ncol = np.ascontiguousarray(ncol, dtype=np.int32)
    if coef.shape != (Yd.shape[1], int(nfolds), npen, nl, p + 1) or ncol.shape != (m, npen):
        raise ValueError("coef must be [m, nfolds, npen, nl, p + 1] and ncol [m, npen]")
    fd = torch.as_tensor(np.ascontiguousarray(foldid, dtype=np.int32), device=x.device)
    triples = np.zeros((m, K, npen, nl, 3))
    table = None
    lp = rp = fp = tp = None
    if interp is not None:
        left, right, frac = (np.ascontiguousarray(interp[0], dtype=np.int32), np.ascontiguousarray(interp[1], dtype=np.int32),
                             np.ascontiguousarray(interp[2], dtype=np.float64))
        if left.shape != (m, K, npen, nl) or right.shape != left.shape or frac.shape != left.shape:
            raise ValueError("interp must be three arrays [m, nfolds, npen, nl]")
        table = np.full(coef.shape, np.nan)
        lp, rp, fp, tp = _iptr(left), _iptr(right), _dptr(frac), _dptr(table)
    if predmat is not None and (predmat.dtype != torch.float64 or not predmat.is_contiguous() or predmat.numel() != m * npen * nl * n):
        raise ValueError("predmat must be a contiguous float64 device tensor of m npen nl n elements")
    ctx = context(x.device.index) if ctx is None else ctx
    torch.cuda.current_stream(x.device).synchronize()
    L.check(L.lib().oemgpu_selftest_cv_score_multi_dev(ctx, ptr, n, ld, p, Yd.data_ptr(), rs, cs, m, fd.data_ptr(), K, _dptr(coef), npen, nl,
                                                       _iptr(ncol), int(type_measure == "mae"), int(nb), lp, rp, fp, tp, _dptr(triples),
                                                       predmat.data_ptr() if predmat is not None else None))
    return triples, table


def _cv_multi_call(x, Y, fid, nfolds, a, standardize, intercept, type_measure, keep, fold_fits=False):
    """oemgpu_cv_dense_multi_dev / _rm_dev -> a dict of the arrays it fills (include/oemgpu.h has their shapes); "outputs" is the
    _ManyOut behind beta, lambda, niter, loss and d"""
    import torch
    n, p = x.shape
    X = _DeviceX(x, _xval_rowmajor_in_place)
    Yd, rs, cs = _device_responses(Y, x.device)
    m, K, npen, nl = Yd.shape[1], int(nfolds), a.npen, a.nl
    fd = torch.as_tensor(fid, device=x.device)
    out = _ManyOut(m, a, p + 1)
    o = {"beta": out.beta, "lambda": out.lam_out, "niter": out.niter, "loss": out.loss, "d": out.d, "outputs": out,
         "ncol": np.zeros((m, npen), dtype=np.int32), "triples": np.zeros((m, K, npen, nl, 3)),
         "fold_n": np.zeros(K, dtype=np.int64), "route": np.zeros(m, dtype=np.int32)}
    if fold_fits:
        o.update({"fold_beta": np.zeros((m, K, npen, nl, p + 1)), "fold_lambda": np.zeros((m, K, npen, nl)),
                  "fold_niter": np.zeros((m, K, npen, nl), dtype=np.int32)})
    if keep:
        o["predmat"] = np.zeros((m, npen, nl, n))
    ctx = context(x.device.index)
    torch.cuda.current_stream(x.device).synchronize()
    X.call("cv_dense_multi", ctx, Yd.data_ptr(), rs, cs, m, fd.data_ptr(), K, int(standardize), int(intercept), int(type_measure == "mae"),
           C.byref(a.c), *out.pointers(), _iptr(o["ncol"]),
           _dptr(o["triples"]), o["fold_n"].ctypes.data_as(C.POINTER(C.c_int64)), _iptr(o["route"]),
           _dptr(o["fold_beta"]) if fold_fits else None, _dptr(o["fold_lambda"]) if fold_fits else None,
           _iptr(o["fold_niter"]) if fold_fits else None, _dptr(o["predmat"]) if keep else None)
    return o


def cv_oem_multi(x, Y, penalty=None, lambda_=None, type_measure=None, nfolds=10, foldid=None, grouped=True, keep=False, rng=None, **kw):
    """cv.oem (family = "gaussian") for m responses on one resident x: [cv_oem(x, Y[:, r], foldid=foldid, ...) for r in range(m)] from
    one fold layout, one gather of x, one set of fold Gram passes, one X'Y pass over the fold-ordered rows, the (K + 1) m fits -- every
    one on its own standardisation and lambda grid, as oem() fits the kept rows -- in batched launches, the fold tables interpolated
    onto every full fit's grid and the held-out rows scored on the device (include/oemgpu.h: oemgpu_cv_dense_multi_dev).
    x: a dense torch device tensor, n x p with n > p >= 2, taken as xval_oem_multi takes it (column-major float64 and row-major float64
    / float32 read in place).  Y: n x m, taken as oem_multi takes it.  foldid (values 1..nfolds; drawn once with `rng` when None) and a
    user lambda_ are shared by all responses; **kw are oem()'s options, as cv_oem passes them.  Returns a list of m results with
    cv_oem's keys (predict_cv, plot_cv and summary_cv take them) and one more, `route`: 0 the response's K + 1 fits ran in a batched
    launch, 1 they were solved one after another inside the call, 2 one of them advised the shifted moment pass and the response went
    through cv_oem() itself.  ValueErrors before any device work: a host or sparse x, weights, ngpus / devices, "ols", family =
    "binomial", n <= p, a Y that is not n x m, len(lambda_) < 2, nfolds < 3, a fold that keeps no more rows than columns."""
    who = "cv_oem_multi()"
    host_or_sparse = (who + " takes a dense torch tensor on a GPU: a host or sparse x is cross-validated one response at a time with cv_oem()")
    if isinstance(x, SparseX) or _is_scipy_sparse(x) or _is_torch_sparse(x):
        raise ValueError(host_or_sparse)
    family = kw.pop("family", "gaussian")
    if family not in ("gaussian", "binomial"):
        raise ValueError("'arg' should be one of 'gaussian', 'binomial'")
    if family == "binomial":
        raise ValueError(who + " serves family = \"gaussian\": binomial responses are cross-validated with cv_oem_logistic_multi()")
    penalty = _match_penalty(penalty)
    type_measure = _check_type_measure(type_measure)
    if lambda_ is not None and len(lambda_) < 2:
        raise ValueError("Need more than one value of lambda for cv.oem")
    if len(kw.pop("weights", ())) > 0:
        raise ValueError(who + ": no observation weights (cv_oem() has none for family = \"gaussian\" either; xval_oem(weights=) cross-validates a weighted response)")
    if kw.get("ngpus") or kw.get("devices") is not None:
        raise ValueError(who + ": the rows of a resident x are not split over devices (ngpus / devices); cv_oem() on a host x takes them")
    if "ols" in penalty:
        raise ValueError(who + ": the \"ols\" penalty is not served; cv_oem() takes it, one response at a time")
    kw.pop("parallel", None)                                      # (cv_oem's resident route accepts and ignores it)
    if getattr(Y, "ndim", None) != 2:
        raise ValueError("Y must be a matrix of n rows and one column per response")
    if getattr(x, "ndim", 0) != 2:
        raise ValueError("x must have at least two columns")
    n, p = x.shape
    m = int(Y.shape[1])
    if m < 1:
        raise ValueError("Y must have at least one column")
    if Y.shape[0] != n:
        raise ValueError("x and y lengths do not match")
    if n <= p:
        raise ValueError(who + " serves n > p only: with n <= p cross-validate each column with cv_oem(x, Y[:, r])")
    if p < 2:
        raise ValueError("x must have at least two columns")
    foldid, nfolds = _fold_ids(foldid, nfolds, n, rng)
    if len(foldid) != n or not np.issubdtype(foldid.dtype, np.integer) or foldid.min() < 1 or nfolds > 512:
        raise ValueError("foldid must hold one integer in 1..nfolds per row of x, nfolds at most 512")
    kept = n - np.bincount(foldid, minlength=nfolds + 1)[1:]
    if np.any(kept <= p):
        i = int(np.argmax(kept <= p))
        raise ValueError(f"{who}: fold {i + 1} leaves {int(kept[i])} rows for {p} columns; cv_oem() sends such folds to its host loop, "
                         "one response at a time")
    if not _is_torch_cuda(x):
        raise ValueError(host_or_sparse)
    lam_arg = () if lambda_ is None else lambda_
    a, varnames, standardize, intercept = oem(x, Y, penalty=penalty, lambda_=lam_arg, _args_only=True, **kw)
    type_measure = _gaussian_measure(type_measure)
    fid = np.ascontiguousarray(foldid, dtype=np.int32)
    o = _cv_multi_call(x, Y, fid, nfolds, a, standardize, intercept, type_measure, keep)
    grouped = _ungrouped_if_small(n, nfolds, grouped)
    own = np.flatnonzero(o["route"] != 2)
    if len(own):
        cvm_all, cvsd_all = _cv_gaussian_triple_stats_many(o["fold_n"], o["triples"][own], o["ncol"][own, -1], grouped)
    out = [None] * m
    for i, r in enumerate(own):
        fit0 = _decorate(o["outputs"].one(r), penalty, varnames, True, n, p)
        lam = [np.asarray(l, dtype=np.float64) for l in fit0["lambda"]]
        res = _cv_result(fit0, penalty, lam, list(cvm_all[i]), list(cvsd_all[i]), _GAUSSIAN_NAMES[type_measure],
                         [np.ascontiguousarray(pm.T) for pm in o["predmat"][r]] if keep else None, foldid)
        res["route"] = int(o["route"][r])
        out[r] = res
    for r in np.flatnonzero(o["route"] == 2):                        # the single route, with its own shift rule
        with warnings.catch_warnings():
            warnings.filterwarnings("ignore", message=".*grouped=FALSE enforced.*")           # (given once, above)
            res = cv_oem(x, Y[:, int(r)], penalty=penalty, lambda_=lambda_, type_measure=type_measure, nfolds=nfolds, foldid=foldid,
                         grouped=grouped, keep=keep, **kw)
        res["route"] = 2
        out[r] = res
    return out


def predict_cv(fit, newx=None, which_model="best.model", s="lambda.min", **kw):
    """predict.cv.oem, R/methods.R (same selection rules as predict.xval.oem, on the full-data fit `oem.fit`)."""
    if isinstance(s, str):
        if s not in ("lambda.min", "lambda.1se"):
            raise ValueError("'arg' should be one of 'lambda.min', 'lambda.1se'")
        lam = fit[s]
    else:
        lam = s
    if isinstance(which_model, str):
        if which_model == "best.model":
            mod = fit["model.min"] - 1
        else:
            if which_model not in fit["penalty"]:
                raise ValueError(f"Model {which_model} specified, but {which_model} not computed.")
            mod = fit["penalty"].index(which_model)
    else:
        mod = int(which_model)
    return predict(fit["oem.fit"], newx, s=lam, which_model=mod, **kw)


# ------------------------------------------------------------------------------------------ consumers
def predict(fit, newx=None, s=None, which_model=0, type="link"):
    """predict.oem, R/methods.R:48-109 (which_model is 0-based or a penalty name).
    newx: a numpy array, a scipy.sparse matrix or a CPU tensor -- multiplied on the host, a numpy result -- or a torch device tensor or
    an open SparseX: the column choice and the interpolation stay here, the product and the link run where newx lies (_predict_device)
    and the n x ncol result is a tensor on its device."""
    if isinstance(which_model, str):
        if which_model not in fit["penalty"]:
            raise ValueError(f"Model {which_model} specified, but {which_model} not computed.")
        which_model = fit["penalty"].index(which_model)
    if which_model >= len(fit["beta"]):
        raise ValueError(f"Model {which_model + 1} specified, but only {len(fit['beta'])} were computed.")
    nbeta = np.array(fit["beta"][which_model])
    if s is not None:
        lam = np.asarray(fit["lambda"][which_model], dtype=np.float64)
        left, right, frac = _lambda_interp(lam, np.atleast_1d(np.asarray(s, dtype=np.float64)))
        nbeta = nbeta[:, left] * frac + nbeta[:, right] * (1 - frac)
    if type == "coefficients":
        return nbeta
    if type == "nonzero":
        return _nonzero_lists(nbeta)
    if newx is None:
        raise ValueError("A value for 'newx' must be supplied")
    newx = _sparse_tensor_arg(newx)
    if _is_torch_sparse(newx):                                                             # a sparse device tensor: a SparseX for the length of the call
        with SparseX(newx) as sx:
            return _predict_device(sx, nbeta, type if fit.get("family") == "binomial" else "link")
    if isinstance(newx, SparseX) or _is_torch_cuda(newx):                                  # on the device, where newx lies
        return _predict_device(newx, nbeta, type if fit.get("family") == "binomial" else "link")
    if hasattr(newx, "tocsc") and newx.__class__.__module__.startswith("scipy.sparse"):    # a dgCMatrix newx: R multiplies it as it is (R/methods.R:48-109)
        import scipy.sparse as sp
        newx = sp.csc_matrix(newx, dtype=np.float64)
        if newx.shape[1] < nbeta.shape[0]:
            newx = sp.hstack([sp.csc_matrix(np.ones((newx.shape[0], 1))), newx], format="csc")
        nfit = np.asarray(newx @ nbeta)
    else:
        newx = np.asarray(newx, dtype=np.float64)
        if newx.shape[1] < nbeta.shape[0]:
            newx = np.column_stack([np.ones(newx.shape[0]), newx])
        nfit = newx @ nbeta
    if fit.get("family") == "binomial":                # predict.oemfit_binomial, R/methods.R:346-367
        if type == "response":
            return 1.0 / (1.0 + np.exp(-nfit))
        if type == "class":
            return np.where(nfit > 0, 1, 0)
    return nfit


def _predict_rowmajor_in_place(x):
    """The dtype code with which predict() hands a device tensor to oemgpu_predict_rm_dev as it lies, or None: then it goes the
    column-major way (a tensor that is already column-major is read in place there; one strided in its columns, or of another element
    type, through _device_matrix's copy).  No limit on n or p."""
    if x.ndim == 2 and x.stride(0) == 1 and x.stride(1) >= x.shape[0]:
        return None
    return _rowmajor_dtype(x)


_PREDICT_TYPES = {"link": 0, "response": 1, "class": 2}


def _predict_device(newx, nbeta, kind):
    """predict()'s product for a torch device tensor or an open SparseX (oemgpu_predict_dev / _rm_dev / _sparse_res): newx is read where
    it lies and the n x ncol result -- float64, a column-major view of the [ncol][n] buffer the kernel wrote; int64 for "class", as
    np.where gives -- stays on its device.  nbeta: the (interpolated) coefficient table, one column per value of s.  The column rule of
    the host path: a newx with as many columns as nbeta has rows is multiplied as it is, one column fewer gets the intercept."""
    import torch
    sparse = isinstance(newx, SparseX)
    if sparse:
        handle = newx.handle                                           # (a closed SparseX: ValueError)
    elif newx.ndim != 2:
        raise ValueError(f"newx must be a matrix: a 2-d tensor, not one of {newx.ndim} dimensions")
    n, p = int(newx.shape[0]), int(newx.shape[1])
    nbeta = np.asarray(nbeta, dtype=np.float64).reshape(nbeta.shape[0], -1)
    q, ncol = nbeta.shape
    if p == q:
        coef = np.zeros((ncol, p + 1))
        coef[:, 1:] = nbeta.T
    elif p == q - 1:
        coef = np.ascontiguousarray(nbeta.T)
    else:
        raise ValueError(f"newx has {p} columns, but the model takes {q - 1} (or {q} with a column for its first coefficient)")
    if n < 1 or ncol < 1:
        raise ValueError("newx has no rows" if n < 1 else "no model column to predict with")
    if kind not in _PREDICT_TYPES:
        kind = "link"
    device = newx.device
    out = torch.empty((ncol, n), dtype=torch.float64, device=device)
    ctx = context(device.index)
    torch.cuda.current_stream(device).synchronize()
    if sparse:
        L.check(L.lib().oemgpu_predict_sparse_res(ctx, handle, _dptr(coef), ncol, _PREDICT_TYPES[kind], out.data_ptr()))
    else:
        _DeviceX(newx, _predict_rowmajor_in_place).call("predict", ctx, _dptr(coef), ncol, _PREDICT_TYPES[kind], out.data_ptr())
    if kind == "class":
        out = out.to(torch.int64)
    return out.t()


def predict_xval(fit, newx=None, which_model="best.model", s="lambda.min", **kw):
    """predict.xval.oem, R/methods.R:765-807 (which_model: "best.model", a penalty name, or a 0-based index)."""
    if isinstance(s, str):
        if s not in ("lambda.min", "lambda.1se"):
            raise ValueError("'arg' should be one of 'lambda.min', 'lambda.1se'")
        lam = fit[s]
    elif np.isscalar(s) or isinstance(s, (list, tuple, np.ndarray)):
        lam = s
    else:
        raise ValueError("Invalid form for s")
    if isinstance(which_model, str):
        if which_model == "best.model":
            mod = fit["model.min"] - 1
        else:
            if which_model not in fit["penalty"]:
                raise ValueError(f"Model {which_model} specified, but {which_model} not computed.")
            mod = fit["penalty"].index(which_model)
    else:
        mod = int(which_model)
        if mod >= len(fit["cvm"]):
            raise ValueError(f"Model {mod + 1} specified, but only {len(fit['cvm'])} were computed.")
    return predict(fit, newx, s=lam, which_model=mod, **kw)


def _lambda_interp(lam, s):
    """lambda.interp, R/utils.R (glmnet's interpolation)."""
    if len(lam) == 1:
        z = np.zeros(len(s), dtype=int)
        return z, z, np.ones(len(s))
    s = np.clip(s, lam.min(), lam.max())
    k = len(lam)
    sfrac = (lam[0] - s) / (lam[0] - lam[k - 1])
    lamn = (lam[0] - lam) / (lam[0] - lam[k - 1])
    coord = np.interp(sfrac, lamn, np.arange(k))
    left, right = np.floor(coord).astype(int), np.ceil(coord).astype(int)
    den = lamn[left] - lamn[right]
    with np.errstate(invalid="ignore", divide="ignore"):
        sf = np.where(left == right, 1.0, (sfrac - lamn[right]) / den)
    return left, right, sf


def logLik(fit, which_model=0):
    """logLik.oem, R/methods.R:431-482 (gaussian)."""
    if isinstance(which_model, str):
        which_model = fit["penalty"].index(which_model)
    loss = np.atleast_1d(np.asarray(fit["loss"][which_model], dtype=np.float64))
    if np.all(loss == 1e99):
        raise ValueError("oem object needed compute.loss set to TRUE. logLik not returned")
    if fit.get("family") == "binomial":                # logLik.oem, binomial branch: -loss
        return -1.0 * loss
    n = float(fit["nobs"])
    return -0.5 * n * (np.log(2 * np.pi) - np.log(n) + np.log(loss)) - 0.5 * n
