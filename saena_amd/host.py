"""ctypes binding of the host-side mirror (include/saena_c.h).

`HostLib("host")` loads libsaena_host.so (g++, no GPU: partition, layout,
generators); `HostLib("gpu")` loads libsaena_amd.so, which carries the same host
code plus the HIP path.  Both fail loudly when the shared object is missing.
"""
import ctypes as C
import os

import numpy as np

from .capi import OpDesc, SgpuError

_HERE = os.path.dirname(os.path.abspath(__file__))
_VP = C.c_void_p
_PI = C.POINTER(C.c_int)
_PD = C.POINTER(C.c_double)
_PS = C.POINTER(C.c_size_t)

CB_ALLGATHER = C.CFUNCTYPE(C.c_int, _VP, _VP, _VP, C.c_size_t)
CB_ALLTOALLV = C.CFUNCTYPE(C.c_int, _VP, _VP, _PS, _PS, _VP, _PS, _PS)
CB_I64 = C.CFUNCTYPE(C.c_int, _VP, C.POINTER(C.c_long), C.c_int)
CB_F64 = C.CFUNCTYPE(C.c_int, _VP, _PD, C.c_int)

HOST_SYMBOLS = {
    "saena_last_error": (C.c_char_p, []),
    "saena_comm_self": (_VP, []),
    "saena_comm_callbacks": (_VP, [C.c_int, C.c_int, _VP, CB_ALLGATHER, CB_ALLTOALLV, CB_I64, CB_F64]),
    "saena_comm_rccl": (_VP, []),
    "saena_comm_shm": (_VP, [C.c_char_p, C.c_int, C.c_int]),
    "saena_measured_chain_us": (C.c_double, []),
    "saena_comm_test_alltoallv": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "saena_comm_test_allreduce_f64": (C.c_int, [_VP, _VP, C.c_int]),
    "saena_comm_test_allreduce_i64": (C.c_int, [_VP, _VP, C.c_int]),
    "saena_comm_free": (None, [_VP]),
    "saena_matrix_new": (_VP, [_VP]),
    "saena_matrix_free": (None, [_VP]),
    "saena_matrix_set": (C.c_int, [_VP, C.c_int, C.c_int, C.c_double]),
    "saena_matrix_set_many": (C.c_int, [_VP, _PI, _PI, _PD, C.c_long]),
    "saena_matrix_read_file": (C.c_int, [_VP, C.c_char_p, C.c_char_p]),
    "saena_matrix_write_bin": (C.c_int, [_VP, C.c_char_p]),
    "saena_matrix_write_mtx": (C.c_int, [_VP, C.c_char_p]),
    "saena_matrix_set_remove_boundary": (C.c_int, [_VP, C.c_int]),
    "saena_matrix_set_partition_buckets": (C.c_int, [_VP, C.c_int]),
    "saena_matrix_add_duplicates": (C.c_int, [_VP, C.c_int]),
    "saena_matrix_set_eig": (C.c_int, [_VP, C.c_double]),
    "saena_matrix_estimate_eig": (C.c_int, [_VP, C.c_int, _PD]),
    "saena_matrix_assemble": (C.c_int, [_VP]),
    "saena_matrix_assemble_with_split": (C.c_int, [_VP, _PI]),
    "saena_matrix_get_num_rows": (C.c_int, [_VP]),
    "saena_matrix_get_num_local_rows": (C.c_int, [_VP]),
    "saena_matrix_get_nnz": (C.c_long, [_VP]),
    "saena_matrix_get_local_nnz": (C.c_long, [_VP]),
    "saena_matrix_get_split": (C.c_int, [_VP, _PI]),
    "saena_matrix_get_desc": (C.c_int, [_VP, C.POINTER(OpDesc)]),
    "saena_matrix_get_layout_extra": (C.c_int, [_VP, C.POINTER(_PI), C.POINTER(C.POINTER(C.c_long))]),
    "saena_matrix_get_halo_columns": (C.c_int, [_VP, C.POINTER(_PI)]),
    "saena_laplacian3D": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int]),
    "saena_laplacian3D_set_rhs": (C.c_int, [_VP, C.c_int, C.c_int, C.c_int, _PD]),
    "saena_band_matrix": (C.c_int, [_VP, C.c_int, C.c_uint]),
    "saena_matmat": (C.c_int, [_VP, _VP, _VP]),
    "saena_debug_spgemm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, _VP, _VP, C.c_int,
                                     C.POINTER(C.c_long)]),
    "saena_debug_spgemm_result": (C.c_int, [_VP, _VP, _VP]),
    "saena_debug_spgemm_stats": (C.c_int, [_VP, _VP]),
    "saena_debug_spgemm_stats_reset": (None, []),
    "saena_debug_filter": (C.c_int, [C.c_int, _VP, _VP, _VP, C.c_double, C.c_int, C.POINTER(C.c_long)]),
    "saena_debug_filter_result": (C.c_int, [_VP, _VP, _VP]),
    "saena_prolong_new": (_VP, [_VP, C.c_int, C.c_int, _PI, _PI, _PI, _PI, _PD, C.c_long]),
    "saena_restrict_from_prolong": (_VP, [_VP]),
    "saena_transfer_free": (None, [_VP]),
    "saena_transfer_get_desc": (C.c_int, [_VP, C.POINTER(OpDesc)]),
    "saena_transfer_get_local_nnz": (C.c_long, [_VP]),
}



class OptionsC(C.Structure):
    """saena_options_c"""
    _fields_ = [("solver_max_iter", C.c_int), ("relative_tol", C.c_double), ("smoother", C.c_int),
                ("preSmooth", C.c_int), ("postSmooth", C.c_int), ("connStrength", C.c_float),
                ("dynamic_levels", C.c_int), ("max_level", C.c_int), ("float_level", C.c_int),
                ("filter_thre", C.c_double), ("filter_max", C.c_double), ("filter_start", C.c_int), ("filter_rate", C.c_int),
                ("switch_to_dense", C.c_int), ("dense_thre", C.c_float), ("dense_sz_thre", C.c_int)]


HOST_SYMBOLS.update({
    "saena_options_default": (C.c_int, [C.POINTER(OptionsC)]),
    "saena_options_from_file": (C.c_int, [C.c_char_p, C.POINTER(OptionsC)]),
    "saena_amg_new": (_VP, []),
    "saena_amg_free": (None, [_VP]),
    "saena_amg_set_matrix": (C.c_int, [_VP, _VP, C.POINTER(OptionsC)]),
    "saena_amg_update": (C.c_int, [_VP, _VP, C.c_int]),
    "saena_amg_set_device_eig": (C.c_int, [_VP, C.c_int]),
    "saena_amg_set_coarse_solver": (C.c_int, [_VP, C.c_char_p]),
    "saena_amg_set_null_space": (C.c_int, [_VP, C.c_char_p]),
    "saena_amg_num_levels": (C.c_int, [_VP]),
    "saena_amg_level_info": (C.c_int, [_VP, C.c_int, _PI, C.POINTER(C.c_long), C.POINTER(C.c_long), _PD]),
    "saena_amg_level_aggregates": (C.c_int, [_VP, C.c_int, _PI, _PI]),
    "saena_amg_level_desc": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(OpDesc)]),
    "saena_amg_level_split": (C.c_int, [_VP, C.c_int, _PI]),
    "saena_amg_to_device": (C.c_int, [_VP]),
    "saena_amg_device_handle": (_VP, [_VP]),
    "saena_amg_device_op": (_VP, [_VP, C.c_int, C.c_int]),
    "saena_amg_solve": (C.c_int, [_VP, _PD, _PD, _PI, _PD, C.c_int]),
    "saena_amg_solve_pCG": (C.c_int, [_VP, _PD, _PD, _PI, _PD, C.c_int]),
    "saena_amg_solve_pCG_block": (C.c_int, [_VP, _PD, _PD, C.c_int, _PI, _PD, C.c_int]),
    "saena_amg_solve_pFGMRES": (C.c_int, [_VP, _PD, _PD, C.c_int, C.c_int, _PI, _PD, C.c_int]),
    "saena_amg_eigs": (C.c_int, [_VP, _PD, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _PD, _PD, _PD, _PI]),
    "saena_amg_eigs_gen": (C.c_int, [_VP, _VP, _PD, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _PD, _PD, _PD, _PI]),
    "saena_amg_eigs_many": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, _PD, C.c_int, C.c_double, C.c_int, _PD, _PD, _PD, _PI, _PI, _PI]),
    "saena_debug_sym_geig": (C.c_int, [C.c_int, _PD, _PD, _PD, _PD]),
    "saena_debug_sym_geig_sweeps": (C.c_int, []),
})

_libs = {}


def load(which="host"):
    """which: 'host' -> libsaena_host.so, 'gpu' -> libsaena_amd.so"""
    if which not in _libs:
        path = os.path.join(_HERE, "libsaena_host.so" if which == "host" else "libsaena_amd.so")
        if which == "host" and os.environ.get("SAENA_HOST_LIB"):      # tools/sanitize_host.sh: the sanitizer build of the host library
            path = os.environ["SAENA_HOST_LIB"]
        if not os.path.exists(path):
            raise SgpuError(f"{path} is missing: run __graft_entry__.build()")
        L = C.CDLL(path, mode=C.RTLD_GLOBAL)
        for name, (res, args) in HOST_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _libs[which] = L
    return _libs[which]


def sym_geig(A, B, which="host"):
    """A v = w B v through saena_debug_sym_geig -> (status, w, V (columns = vectors), Jacobi sweeps)"""
    L = load(which)
    A, B = _ad(A), _ad(B)
    n = A.shape[0]
    w, V = np.full(n, np.nan), np.full((n, n), np.nan)
    st = L.saena_debug_sym_geig(n, A.ctypes.data_as(_PD), B.ctypes.data_as(_PD), w.ctypes.data_as(_PD), V.ctypes.data_as(_PD))
    return st, w, V, L.saena_debug_sym_geig_sweeps()


def _ai(a):
    return np.ascontiguousarray(a, np.int32)


def _ad(a):
    return np.ascontiguousarray(a, np.float64)


class Comm:
    """Setup-time communicator: self, the GPU runtime's RCCL communicator, the native shared-memory communicator of the
    ranks of one node, or torch.distributed (any backend that moves CPU tensors, e.g. gloo) through callbacks."""

    def __init__(self, which="host", kind="self", dist=None):
        self.L = load(which)
        self.kind = kind
        self.rank, self.nranks = 0, 1
        self._cbs = None
        if kind == "self":
            self.h = self.L.saena_comm_self()
        elif kind == "rccl":
            self.h = self.L.saena_comm_rccl()
            if not self.h:
                raise SgpuError(self.L.saena_last_error().decode())
        elif kind == "shm":              # dist = (name, rank, nranks): the ranks of one node through shared memory (native)
            name, self.rank, self.nranks = dist
            self.h = self.L.saena_comm_shm(str(name).encode(), int(self.rank), int(self.nranks))
            if not self.h:
                raise SgpuError(self.L.saena_last_error().decode())
        elif kind == "dist":
            self.rank, self.nranks = dist.get_rank(), dist.get_world_size()
            self._make_dist_callbacks(dist)
            self.h = self.L.saena_comm_callbacks(self.rank, self.nranks, None, *self._cbs)
        else:
            raise ValueError(kind)

    def _make_dist_callbacks(self, dist):
        import torch
        np_ = self.nranks

        def buf(ptr, n):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n,)) if n else np.zeros(0, np.uint8)

        def allgather(user, send, recv, nbytes):
            try:
                s = torch.from_numpy(buf(send, nbytes).copy())
                outs = [torch.empty(nbytes, dtype=torch.uint8) for _ in range(np_)]
                dist.all_gather(outs, s)
                r = buf(recv, nbytes * np_)
                for q in range(np_):
                    r[q * nbytes:(q + 1) * nbytes] = outs[q].numpy()
                return 0
            except Exception as e:      # pragma: no cover
                print("allgather callback failed:", e)
                return 1

        def alltoallv(user, send, sc, sd, recv, rc, rd):
            try:
                ins = [torch.from_numpy(buf(send + sd[q] if send else None, sc[q]).copy()) if sc[q] else torch.empty(0, dtype=torch.uint8)
                       for q in range(np_)]
                outs = [torch.empty(rc[q], dtype=torch.uint8) for q in range(np_)]
                # pairwise exchange (works on every backend that has send/recv)
                me = self.rank
                outs[me] = ins[me].clone()
                for step in range(1, np_):
                    to, frm = (me + step) % np_, (me - step) % np_
                    reqs = []
                    if sc[to]:
                        reqs.append(dist.isend(ins[to], to))
                    if rc[frm]:
                        reqs.append(dist.irecv(outs[frm], frm))
                    for rq in reqs:
                        rq.wait()
                for q in range(np_):
                    if rc[q]:
                        buf(recv + rd[q], rc[q])[:] = outs[q].numpy()
                return 0
            except Exception as e:      # pragma: no cover
                print("alltoallv callback failed:", e)
                return 1

        def ar_i64(user, v, n):
            t = torch.from_numpy(np.ctypeslib.as_array(v, shape=(n,)).copy())
            dist.all_reduce(t)
            np.ctypeslib.as_array(v, shape=(n,))[:] = t.numpy()
            return 0

        def ar_f64(user, v, n):
            t = torch.from_numpy(np.ctypeslib.as_array(v, shape=(n,)).copy())
            dist.all_reduce(t)
            np.ctypeslib.as_array(v, shape=(n,))[:] = t.numpy()
            return 0

        self._cbs = (CB_ALLGATHER(allgather), CB_ALLTOALLV(alltoallv), CB_I64(ar_i64), CB_F64(ar_f64))


def _check(L, status):
    if status != 0:
        raise SgpuError("saena host: " + L.saena_last_error().decode(errors="replace"))


def desc_arrays(d: OpDesc, nranks_for_scan=None):
    """Copy every array an sgpu_op_desc points at into numpy (for layout tests)."""
    def ai(p, n):
        return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.int32)

    def ad(p, n):
        return np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.float64)

    return dict(
        M=d.M, N_local=d.N_local, col_offset=d.col_offset,
        nnzPerRow_local=ai(d.nnzPerRow_local, d.M), col_local=ai(d.col_local, d.nnz_l_local), val_local=ad(d.val_local, d.nnz_l_local),
        nnzPerCol_remote=ai(d.nnzPerCol_remote, d.col_remote_size), row_remote=ai(d.row_remote, d.nnz_l_remote),
        val_remote=ad(d.val_remote, d.nnz_l_remote),
        recvProcRank=ai(d.recvProcRank, d.numRecvProc), recvProcCount=ai(d.recvProcCount, d.numRecvProc),
        sendProcRank=ai(d.sendProcRank, d.numSendProc), sendProcCount=ai(d.sendProcCount, d.numSendProc),
        vIndex=ai(d.vIndex, d.vIndexSize), inv_diag=ad(d.inv_diag, d.M) if d.inv_diag else None,
    )


class Matrix:
    """saena::matrix mirror (reference include/saena.hpp:14-73)."""

    def __init__(self, comm: Comm):
        self.comm, self.L = comm, comm.L
        self.h = self.L.saena_matrix_new(comm.h)

    def set(self, i, j, v):
        _check(self.L, self.L.saena_matrix_set(self.h, int(i), int(j), float(v)))

    def set_many(self, rows, cols, vals):
        r, c, v = _ai(rows), _ai(cols), _ad(vals)
        _check(self.L, self.L.saena_matrix_set_many(self.h, r.ctypes.data_as(_PI), c.ctypes.data_as(_PI), v.ctypes.data_as(_PD), len(r)))

    def read_file(self, name, input_type=""):
        _check(self.L, self.L.saena_matrix_read_file(self.h, os.fsencode(name), input_type.encode()))
        return self

    def write_bin(self, name):
        _check(self.L, self.L.saena_matrix_write_bin(self.h, os.fsencode(name)))

    def write_mtx(self, name):
        """saena::matrix::writeMatrixToFile: this rank's entries as <name>-r<rank>.mtx"""
        _check(self.L, self.L.saena_matrix_write_mtx(self.h, os.fsencode(name)))

    def set_remove_boundary(self, flag):
        self.L.saena_matrix_set_remove_boundary(self.h, 1 if flag else 0)

    def set_partition_buckets(self, n):
        """opt-in: at least n row buckets in the nnz-balanced partition of assemble() instead of the reference's nparts^2"""
        _check(self.L, self.L.saena_matrix_set_partition_buckets(self.h, int(n)))
        return self

    def laplacian3D(self, mx, my=None, mz=None):
        my = mx if my is None else my
        mz = mx if mz is None else mz
        self._grid = (mx, my, mz)
        _check(self.L, self.L.saena_laplacian3D(self.h, mx, my, mz))
        return self

    def band_matrix(self, M, bw):
        _check(self.L, self.L.saena_band_matrix(self.h, M, bw))
        return self

    def set_eig(self, eig):
        """saena::matrix::set_eig(double): the Chebyshev eig_max of this matrix, kept by set_matrix and the updates as it is"""
        _check(self.L, self.L.saena_matrix_set_eig(self.h, float(eig)))
        return self

    def estimate_eig(self, steps=20):
        """the value set_eig takes, estimated on the device (saena_matrix_estimate_eig; GPU library, one rank); nothing is stored"""
        v = C.c_double()
        _check(self.L, self.L.saena_matrix_estimate_eig(self.h, int(steps), C.byref(v)))
        return v.value

    def assemble(self, split=None):
        if split is None:
            _check(self.L, self.L.saena_matrix_assemble(self.h))
        else:
            s = _ai(split)
            _check(self.L, self.L.saena_matrix_assemble_with_split(self.h, s.ctypes.data_as(_PI)))
        return self

    def matmat(self, B):
        """saena::amg::matmat: C = self * B (host SpGEMM, one rank)"""
        Cm = Matrix(self.comm)
        _check(self.L, self.L.saena_matmat(self.h, B.h, Cm.h))
        return Cm

    def laplacian3D_rhs(self):
        mx, my, mz = self._grid
        out = np.empty(self.num_local_rows)
        _check(self.L, self.L.saena_laplacian3D_set_rhs(self.h, mx, my, mz, out.ctypes.data_as(_PD)))
        return out

    @property
    def num_rows(self):
        return self.L.saena_matrix_get_num_rows(self.h)

    @property
    def num_local_rows(self):
        return self.L.saena_matrix_get_num_local_rows(self.h)

    @property
    def nnz(self):
        return self.L.saena_matrix_get_nnz(self.h)

    @property
    def local_nnz(self):
        return self.L.saena_matrix_get_local_nnz(self.h)

    @property
    def split(self):
        s = np.zeros(self.comm.nranks + 1, np.int32)
        _check(self.L, self.L.saena_matrix_get_split(self.h, s.ctypes.data_as(_PI)))
        return s

    def desc(self):
        d = OpDesc()
        _check(self.L, self.L.saena_matrix_get_desc(self.h, C.byref(d)))
        return d

    def layout(self):
        d = self.desc()
        out = desc_arrays(d)
        cr, sc = _PI(), C.POINTER(C.c_long)()
        self.L.saena_matrix_get_layout_extra(self.h, C.byref(cr), C.byref(sc))
        out["col_remote"] = np.ctypeslib.as_array(cr, shape=(d.nnz_l_remote,)).copy() if d.nnz_l_remote else np.zeros(0, np.int32)
        out["nnzPerProcScan"] = np.ctypeslib.as_array(sc, shape=(self.comm.nranks + 1,)).copy()
        return out

    def halo_columns(self):
        """global column id of every slot of this rank's receive (halo) buffer"""
        d = self.desc()
        p = _PI()
        self.L.saena_matrix_get_halo_columns(self.h, C.byref(p))
        return np.ctypeslib.as_array(p, shape=(d.col_remote_size,)).copy() if d.col_remote_size else np.zeros(0, np.int32)

    def free(self):
        if self.h:
            self.L.saena_matrix_free(self.h)
            self.h = None


class Transfer:
    """prolong_matrix / restrict_matrix mirror."""

    def __init__(self, comm, h):
        self.comm, self.L, self.h = comm, comm.L, h

    @classmethod
    def prolong(cls, comm, Mbig, Nbig, split_row, split_col, rows, cols, vals):
        sr, sc, r, c, v = _ai(split_row), _ai(split_col), _ai(rows), _ai(cols), _ad(vals)
        h = comm.L.saena_prolong_new(comm.h, Mbig, Nbig, sr.ctypes.data_as(_PI), sc.ctypes.data_as(_PI),
                                     r.ctypes.data_as(_PI), c.ctypes.data_as(_PI), v.ctypes.data_as(_PD), len(r))
        if not h:
            raise SgpuError(comm.L.saena_last_error().decode())
        return cls(comm, h)

    def transpose(self):
        h = self.L.saena_restrict_from_prolong(self.h)
        if not h:
            raise SgpuError(self.L.saena_last_error().decode())
        return Transfer(self.comm, h)

    def desc(self):
        d = OpDesc()
        _check(self.L, self.L.saena_transfer_get_desc(self.h, C.byref(d)))
        return d

    def layout(self):
        return desc_arrays(self.desc())


# the counters of saena_debug_spgemm_stats, in its order (include/saena_c.h)
SPGEMM_STATS = ("host_dense", "host_hash", "host_rehash", "light", "medium", "try_kept", "try_abandoned", "lds", "hbm",
                "chunks", "windows", "declined", "on_device")
SPGEMM_MODES = {"auto": 0, "host": 1, "device": 2}


def spgemm(L, a_ptr, a_col, a_val, b_ptr, b_col, b_val, b_cols, row_offset=0, mode="auto", split_row=None):
    """C = A B through the products of the AMG setup (saena_debug_spgemm): -> (c_ptr, c_col, c_val).
    A is (len(a_ptr) - 1) x (len(b_ptr) - 1), B has b_cols columns; the columns of every row of B must be distinct and
    ascending.  mode: "host" = the host kernel, "device" = the GPU kernel whatever the size (SgpuError when it is missing
    or declines), "auto" = what the setup does.  split_row: hand B over in two pieces, rows [0, split_row) and the rest,
    as the distributed setup holds its own and its fetched rows."""
    ap, ac, av = np.ascontiguousarray(a_ptr, np.int64), _ai(a_col), _ad(a_val)
    bp, bc, bv = np.ascontiguousarray(b_ptr, np.int64), _ai(b_col), _ad(b_val)
    if len(ac) != ap[-1] or len(av) != ap[-1] or len(bc) != bp[-1] or len(bv) != bp[-1]:
        raise ValueError("spgemm: array lengths do not match the row pointers")
    ptr = lambda a: a.ctypes.data_as(_VP)
    if split_row is None:
        pieces = (ptr(bc), ptr(bv), 0, None, None)
    else:
        cut = int(bp[split_row])
        c0, v0, c1, v1 = bc[:cut].copy(), bv[:cut].copy(), bc[cut:].copy(), bv[cut:].copy()      # two allocations, as in the setup
        pieces = (ptr(c0), ptr(v0), cut, ptr(c1), ptr(v1))
    n = C.c_long()
    _check(L, L.saena_debug_spgemm(SPGEMM_MODES[mode], len(ap) - 1, len(bp) - 1, int(b_cols), ptr(ap), ptr(ac), ptr(av), ptr(bp), *pieces,
                                   int(row_offset), C.byref(n)))
    c_ptr, c_col, c_val = np.zeros(len(ap), np.int64), np.zeros(n.value, np.int32), np.zeros(n.value, np.float64)
    _check(L, L.saena_debug_spgemm_result(ptr(c_ptr), ptr(c_col), ptr(c_val)))
    return c_ptr, c_col, c_val


def spgemm_stats(L, total=False):
    """which path served the rows of the last product (total: of every product since spgemm_stats_reset) -> dict"""
    last, tot = np.zeros(len(SPGEMM_STATS), np.int64), np.zeros(len(SPGEMM_STATS), np.int64)
    n = L.saena_debug_spgemm_stats(last.ctypes.data_as(_VP), tot.ctypes.data_as(_VP))
    if n != len(SPGEMM_STATS):
        raise SgpuError(f"saena_debug_spgemm_stats has {n} counters, the binding names {len(SPGEMM_STATS)}")
    return dict(zip(SPGEMM_STATS, (int(x) for x in (tot if total else last))))


def spgemm_stats_reset(L):
    L.saena_debug_spgemm_stats_reset()


def filter_csr(L, ptr, col, val, thre, row_offset=0):
    """the setup's filter on rows [row_offset, row_offset + len(ptr) - 1) of a level (saena_debug_filter): entries with
    |v| <= thre off the diagonal are lumped into it -> (ptr, col, val)"""
    p, c, v = np.ascontiguousarray(ptr, np.int64), _ai(col), _ad(val)
    if len(c) != p[-1] or len(v) != p[-1]:
        raise ValueError("filter_csr: array lengths do not match the row pointers")
    at = lambda a: a.ctypes.data_as(_VP)
    n = C.c_long()
    _check(L, L.saena_debug_filter(len(p) - 1, at(p), at(c), at(v), float(thre), int(row_offset), C.byref(n)))
    o_ptr, o_col, o_val = np.zeros(len(p), np.int64), np.zeros(n.value, np.int32), np.zeros(n.value, np.float64)
    _check(L, L.saena_debug_filter_result(at(o_ptr), at(o_col), at(o_val)))
    return o_ptr, o_col, o_val


def device_operator(obj, halo_fp32=False):
    """sgpu_op_create from a host Matrix/Transfer (GPU library only)."""
    from . import capi
    d = obj.desc()
    d.halo_fp32 = 1 if halo_fp32 else 0
    op = capi.Operator.__new__(capi.Operator)
    h = _VP()
    capi.check(capi.lib().sgpu_op_create(C.byref(d), C.byref(h)))
    op.h, op.M, op.N_local, op._keep = h, d.M, d.N_local, None
    return op


def options(L, xml=None, **kw):
    """saena::options: defaults (saena.hpp:151-155), an options XML of the reference's format, then overrides"""
    o = OptionsC()
    L.saena_options_default(C.byref(o))
    if xml is not None:
        _check(L, L.saena_options_from_file(os.fsencode(xml), C.byref(o)))
    for k, v in kw.items():
        if k == "smoother":
            v = 0 if v == "jacobi" else 1
        setattr(o, k, v)
    return o


# the reference's data/options001.xml (Jacobi 3+3, tol 1e-8, conn_str 0.2, filter 1e-14 -> 1e-8 rate 2)
OPTIONS001 = dict(solver_max_iter=50, relative_tol=1e-8, smoother="jacobi", preSmooth=3, postSmooth=3, connStrength=0.2,
                  dynamic_levels=1, max_level=20, float_level=3, filter_thre=1e-14, filter_max=1e-8, filter_start=1, filter_rate=2)


class AmgSolver:
    """saena::amg mirror (reference include/saena.hpp:195-265): set_matrix on the host, solve on the GPU."""

    def __init__(self, A: Matrix, opts: OptionsC, device_eig=None, coarse_solver=None, null_space=None):
        """device_eig: True lets the one-rank setup and the updates take eig_max from the device estimate (saena_amg_set_device_eig);
        None leaves the library's default (off, unless SAENA_DEVICE_EIG=1).
        coarse_solver: "direct", "cg" or "device_cg" (saena_amg_set_coarse_solver), read by to_device; None leaves the library's
        default ("direct", unless SAENA_COARSE_SOLVER names another)
        null_space: "constant" (saena_amg_set_null_space), read by to_device: A annihilates constants (assemble it after
        set_remove_boundary(False)); the solves solve A u = rhs - mean(rhs) and return the solution of zero mean, eigs the smallest
        nonzero pairs.  None / "none": the solver as ever"""
        self.A, self.L = A, A.L
        self.h = self.L.saena_amg_new()
        if device_eig is not None:
            self.set_device_eig(device_eig)
        if coarse_solver is not None:
            self.set_coarse_solver(coarse_solver)
        if null_space is not None:
            self.set_null_space(null_space)
        _check(self.L, self.L.saena_amg_set_matrix(self.h, A.h, C.byref(opts)))
        self.opts = opts

    def set_device_eig(self, on):
        _check(self.L, self.L.saena_amg_set_device_eig(self.h, 1 if on else 0))
        return self

    def set_coarse_solver(self, name):
        _check(self.L, self.L.saena_amg_set_coarse_solver(self.h, str(name).encode()))
        return self

    def set_null_space(self, name):
        _check(self.L, self.L.saena_amg_set_null_space(self.h, str(name).encode()))
        return self

    def update(self, A_new: Matrix, mode):
        """saena::amg::update1 / update2 (saena_amg_update): A_new, of the same size, becomes level 0 of the built hierarchy.  mode 1:
        nothing else changes; mode 2: every coarse operator is rebuilt over the kept aggregates, P and R.  One rank.  A hierarchy
        that is on the device gets new device operators for the refreshed levels.  A_new must stay alive; a refusal raises and
        leaves the hierarchy as it was."""
        _check(self.L, self.L.saena_amg_update(self.h, A_new.h, int(mode)))
        self.A = A_new
        return self

    @property
    def num_levels(self):
        return self.L.saena_amg_num_levels(self.h)

    def level_aggregates(self, l):
        """coarse id of every fine row of level l (one-rank setups), and the number of aggregates"""
        rows = self.level_info(l)["rows"]
        out, n = np.zeros(rows, np.int32), C.c_int()
        _check(self.L, self.L.saena_amg_level_aggregates(self.h, l, out.ctypes.data_as(_PI), C.byref(n)))
        return out, n.value

    def level_info(self, l):
        rows, na, npp, eig = C.c_int(), C.c_long(), C.c_long(), C.c_double()
        _check(self.L, self.L.saena_amg_level_info(self.h, l, C.byref(rows), C.byref(na), C.byref(npp), C.byref(eig)))
        return dict(rows=rows.value, nnzA=na.value, nnzP=npp.value, eig_max=eig.value)

    def level_split(self, l):
        s = np.zeros(self.A.comm.nranks + 1, np.int32)
        _check(self.L, self.L.saena_amg_level_split(self.h, l, s.ctypes.data_as(_PI)))
        return s

    def level_layout(self, l, which):
        d = OpDesc()
        _check(self.L, self.L.saena_amg_level_desc(self.h, l, which, C.byref(d)))
        return desc_arrays(d)

    def to_device(self):
        _check(self.L, self.L.saena_amg_to_device(self.h))
        return self

    def device_handle(self):
        return self.L.saena_amg_device_handle(self.h)

    def device_op(self, l, which=0):
        from . import capi
        op = capi.Operator.__new__(capi.Operator)
        op.h = _VP(self.L.saena_amg_device_op(self.h, l, which))
        info = None
        op._keep = None
        op.destroy = lambda: None          # owned by the solver
        info = op.info()
        op.M, op.N_local = info["M"], info["N_local"]
        return op

    def _solve(self, fn, rhs, cap=256):
        rhs = _ad(rhs)
        u = np.zeros_like(rhs)
        it = C.c_int()
        hist = np.full(cap, np.nan)
        st = fn(self.h, rhs.ctypes.data_as(_PD), u.ctypes.data_as(_PD), C.byref(it), hist.ctypes.data_as(_PD), cap)
        if st not in (0, -6):
            _check(self.L, st)
        return u, it.value, hist[~np.isnan(hist)], st == 0

    def solve(self, rhs):
        return self._solve(self.L.saena_amg_solve, rhs)

    def solve_pCG(self, rhs):
        return self._solve(self.L.saena_amg_solve_pCG, rhs)

    def solve_pFGMRES(self, rhs, restart=30, precond=True, cap=4096):
        """restarted flexible GMRES (saena_amg_solve_pFGMRES) -> (u, inner iterations, residual estimates, converged)"""
        return self._solve(lambda h, r, u, it, hist, c: self.L.saena_amg_solve_pFGMRES(h, r, u, int(restart), 1 if precond else 0, it, hist, c), rhs, cap=cap)

    def solve_pCG_block(self, rhs, cap=256):
        """rhs: (n, K) with K = 2, 4 or 8 -> (u (n, K), iters[K], [history of column j], converged): saena_amg_solve_pCG_block"""
        rhs = np.asfortranarray(rhs, np.float64)                 # column-major n x K
        n, K = rhs.shape
        u = np.zeros((n, K), order="F")
        it = (C.c_int * K)()
        hist = np.full((K, cap), np.nan)
        st = self.L.saena_amg_solve_pCG_block(self.h, rhs.ctypes.data_as(_PD), u.ctypes.data_as(_PD), K, it, hist.ctypes.data_as(_PD), cap)
        if st not in (0, -6):
            _check(self.L, st)
        return u, [int(v) for v in it], [h[~np.isnan(h)] for h in hist], st == 0

    def eigs(self, K, nev, x0=None, max_iter=100, tol=1e-8, precond=True, B=None):
        """the nev smallest eigenpairs by LOBPCG on K = 2, 4 or 8 vectors (saena_amg_eigs); x0: (n, K) start vectors or None for the
        default start.  With B (an assembled Matrix of the same size) the generalised problem A x = lambda B x (saena_amg_eigs_gen):
        X is B-orthonormal on return.  A lumped (diagonal) B is assembled after B.set_remove_boundary(False), or assemble() removes
        its single-entry rows as boundary nodes -> (lambda[K], X (n, K), res[K], iterations, converged)"""
        n = self.A.num_local_rows
        p0 = None
        if x0 is not None:
            x0 = np.asfortranarray(x0, np.float64)
            assert x0.shape == (n, K), x0.shape
            p0 = x0.ctypes.data_as(_PD)
        X = np.zeros((n, K), order="F")
        lam, res, it = np.full(K, np.nan), np.full(K, np.nan), C.c_int()
        if B is None:
            st = self.L.saena_amg_eigs(self.h, p0, int(K), int(nev), int(max_iter), float(tol), 1 if precond else 0, lam.ctypes.data_as(_PD),
                                       X.ctypes.data_as(_PD), res.ctypes.data_as(_PD), C.byref(it))
        else:
            st = self.L.saena_amg_eigs_gen(self.h, B.h, p0, int(K), int(nev), int(max_iter), float(tol), 1 if precond else 0,
                                           lam.ctypes.data_as(_PD), X.ctypes.data_as(_PD), res.ctypes.data_as(_PD), C.byref(it))
        if st not in (0, -6):
            _check(self.L, st)
        return lam, X, res, it.value, st == 0

    def eigs_many(self, nev, K=8, sweep_nev=0, x0=None, max_iter=400, tol=1e-8, precond=True, B=None):
        """more than K eigenpairs (saena_amg_eigs_many): the nev <= 64 smallest pairs of A x = lambda x, or of A x = lambda B x with B (an
        assembled Matrix of the same size, as in eigs), by sweeps of LOBPCG on K = 2, 4 or 8 vectors with converged vectors locked; a
        sweep asks for sweep_nev pairs (0: K / 2).  max_iter bounds the total over all sweeps; x0: (n, K) start vectors or None for
        generated ones -> (lambda[found], Q (n, found), res[found], total iterations, sweeps, converged); found = nev when converged"""
        n = self.A.num_local_rows
        p0 = None
        if x0 is not None:
            x0 = np.asfortranarray(x0, np.float64)
            assert x0.shape == (n, K), x0.shape
            p0 = x0.ctypes.data_as(_PD)
        Q = np.zeros((n, max(1, nev)), order="F")
        lam, res = np.full(max(1, nev), np.nan), np.full(max(1, nev), np.nan)
        it, nl, sw = C.c_int(), C.c_int(), C.c_int()
        st = self.L.saena_amg_eigs_many(self.h, B.h if B is not None else None, int(nev), int(K), int(sweep_nev), p0, int(max_iter), float(tol),
                                        1 if precond else 0, lam.ctypes.data_as(_PD), Q.ctypes.data_as(_PD), res.ctypes.data_as(_PD), C.byref(it),
                                        C.byref(nl), C.byref(sw))
        if st not in (0, -6):
            _check(self.L, st)
        L = nl.value
        return lam[:L], Q[:, :L], res[:L], it.value, sw.value, st == 0

    def free(self):
        if self.h:
            self.L.saena_amg_free(self.h)
            self.h = None
