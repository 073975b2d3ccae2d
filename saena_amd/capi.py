"""ctypes binding of libsaena_amd.so (include/saena_gpu.h).

There is no CPU fallback: importing works anywhere (so the symbol table can be
checked without a GPU), but every compute entry point needs `init()` to have
found an MI355X, and a missing shared library raises immediately.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsaena_amd.so")

_PI = C.POINTER(C.c_int)
_PD = C.POINTER(C.c_double)


class SgpuError(RuntimeError):
    pass


class OpDesc(C.Structure):
    """sgpu_op_desc (include/saena_gpu.h)"""
    _fields_ = [
        ("M", C.c_int), ("N_local", C.c_int), ("col_offset", C.c_int),
        ("nnz_l_local", C.c_long), ("nnzPerRow_local", _PI), ("col_local", _PI), ("val_local", _PD),
        ("nnz_l_remote", C.c_long), ("col_remote_size", C.c_int),
        ("nnzPerCol_remote", _PI), ("row_remote", _PI), ("val_remote", _PD),
        ("numRecvProc", C.c_int), ("numSendProc", C.c_int),
        ("recvProcRank", _PI), ("recvProcCount", _PI), ("sendProcRank", _PI), ("sendProcCount", _PI),
        ("vIndexSize", C.c_int), ("vIndex", _PI), ("inv_diag", _PD), ("halo_fp32", C.c_int),
    ]


class AmgParams(C.Structure):
    """sgpu_amg_params"""
    _fields_ = [
        ("preSmooth", C.c_int), ("postSmooth", C.c_int), ("smoother", C.c_int), ("jacobi_omega", C.c_double),
        ("coarse_solver", C.c_int), ("CG_coarsest_max_iter", C.c_int), ("CG_coarsest_tol", C.c_double),
        ("solver_max_iter", C.c_int), ("solver_tol", C.c_double), ("use_graph", C.c_int),
    ]


# every symbol include/saena_gpu.h (the boundary) and include/saena_gpu_debug.h (test scaffolding) declare:
# name -> (restype, argtypes)
_VP = C.c_void_p
SYMBOLS = {
    "sgpu_last_error": (C.c_char_p, []),
    "sgpu_get_unique_id": (C.c_int, [_VP]),
    "sgpu_init": (C.c_int, [C.c_int, C.c_int, C.c_int, _VP]),
    "sgpu_finalize": (C.c_int, []),
    "sgpu_rank": (C.c_int, []),
    "sgpu_nranks": (C.c_int, []),
    "sgpu_device_sync": (C.c_int, []),
    "sgpu_barrier": (C.c_int, []),
    "sgpu_vec_alloc": (C.c_int, [C.POINTER(_VP), C.c_size_t]),
    "sgpu_vec_free": (C.c_int, [_VP]),
    "sgpu_vec_upload": (C.c_int, [_VP, _VP, C.c_size_t]),
    "sgpu_vec_download": (C.c_int, [_VP, _VP, C.c_size_t]),
    "sgpu_vec_fill": (C.c_int, [_VP, C.c_double, C.c_size_t]),
    "sgpu_vec_copy": (C.c_int, [_VP, _VP, C.c_size_t]),
    "sgpu_vec_axpby": (C.c_int, [C.c_double, _VP, C.c_double, _VP, C.c_size_t]),
    "sgpu_dot": (C.c_int, [_VP, _VP, C.c_size_t, _PD]),
    "sgpu_vec_center": (C.c_int, [_VP, _VP, C.c_size_t, _PD]),
    "sgpu_block_center": (C.c_int, [_VP, _VP, C.c_size_t, C.c_int]),
    "sgpu_op_create": (C.c_int, [C.POINTER(OpDesc), C.POINTER(_VP)]),
    "sgpu_op_destroy": (C.c_int, [_VP]),
    "sgpu_op_info": (C.c_int, [_VP, _PI, _PI, C.POINTER(C.c_long), C.POINTER(C.c_long), _PI, _PI]),
    "sgpu_op_set_lanes_per_row": (C.c_int, [_VP, C.c_int]),
    "sgpu_op_set_variant": (C.c_int, [_VP, C.c_int]),
    "sgpu_op_autotune": (C.c_int, [_VP]),
    "sgpu_op_get_variant": (C.c_int, [_VP, _PI, C.POINTER(C.c_char_p)]),
    "sgpu_op_set_x_windows": (C.c_int, [_VP, C.c_int]),
    "sgpu_op_get_x_windows": (C.c_int, [_VP, _PI]),
    "sgpu_op_get_x_window_kernel": (C.c_int, [_VP, _PI]),
    "sgpu_op_get_x_window_code_width": (C.c_int, [_VP, _PI]),
    "sgpu_op_get_x_window_row_format": (C.c_int, [_VP, _PI]),
    "sgpu_spmv": (C.c_int, [_VP, _VP, _VP]),
    "sgpu_residual": (C.c_int, [_VP, _VP, _VP, _VP]),
    "sgpu_residual_negative": (C.c_int, [_VP, _VP, _VP, _VP]),
    "sgpu_residual_multiply": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_double]),
    "sgpu_jacobi": (C.c_int, [_VP, C.c_int, C.c_double, _VP, _VP]),
    "sgpu_chebyshev": (C.c_int, [_VP, C.c_int, C.c_double, _VP, _VP]),
    "sgpu_prolong_correct": (C.c_int, [_VP, _VP, _VP]),
    "sgpu_op_eig_max": (C.c_int, [_VP, C.c_int, _PD]),
    "sgpu_debug_capture": (C.c_int, [C.c_int]),
    "sgpu_debug_dcg_matvec_time": (C.c_int, [_VP, _VP, _VP, C.c_int, C.POINTER(C.c_float)]),
    "sgpu_debug_pack": (C.c_int, [_VP, _VP, _PD]),
    "sgpu_debug_gather_probe": (C.c_int, [_VP, C.c_int, _VP, C.c_int, C.POINTER(C.c_float)]),
    "sgpu_debug_block_plan": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_long)]),
    "sgpu_debug_stream_ceiling": (C.c_int, [C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "sgpu_debug_inject_halo": (C.c_int, [_VP, _PD]),
    "sgpu_debug_pack_block": (C.c_int, [_VP, _VP, C.c_int, _PD]),
    "sgpu_debug_inject_halo_block": (C.c_int, [_VP, C.c_int, _PD]),
    "sgpu_spmv_host": (C.c_int, [_VP, _PD, _PD]),
    "sgpu_jacobi_host": (C.c_int, [_VP, C.c_int, C.c_double, _PD, _PD]),
    "sgpu_chebyshev_host": (C.c_int, [_VP, C.c_int, C.c_double, _PD, _PD]),
    "sgpu_amg_default_params": (C.c_int, [C.POINTER(AmgParams)]),
    "sgpu_amg_create": (C.c_int, [C.c_int, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP), _PD, C.POINTER(AmgParams), C.POINTER(_VP)]),
    "sgpu_amg_create_null_space": (C.c_int, [C.c_int, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP), _PD, C.POINTER(AmgParams), C.c_int,
                                             C.POINTER(_VP)]),
    "sgpu_amg_get_null_space": (C.c_int, [_VP, _PI]),
    "sgpu_amg_destroy": (C.c_int, [_VP]),
    "sgpu_vcycle": (C.c_int, [_VP, _VP, _VP]),
    "sgpu_solve": (C.c_int, [_VP, _VP, _VP, _PI, _PD, C.c_int]),
    "sgpu_solve_pCG": (C.c_int, [_VP, _VP, _VP, _PI, _PD, C.c_int]),
    "sgpu_solve_CG": (C.c_int, [_VP, _VP, _VP, _PI, _PD, C.c_int]),
    "sgpu_solve_smoother": (C.c_int, [_VP, _VP, _VP, _PI, _PD, C.c_int]),
    "sgpu_amg_set_solve_params": (C.c_int, [_VP, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int]),
    "sgpu_amg_profile_matvecs": (C.c_int, [_VP, C.c_int, _PD]),
    "sgpu_amg_set_operator": (C.c_int, [_VP, C.c_int, _VP, C.c_double]),
    "sgpu_coarsest_solve": (C.c_int, [_VP, _VP, _VP, _PI]),
    "sgpu_debug_on_fatal_print": (C.c_int, [C.c_char_p]),
    "sgpu_debug_launch_count": (C.c_int, [C.POINTER(C.c_long)]),
    "sgpu_debug_op_storage": (C.c_int, [_VP, C.POINTER(C.c_uint), C.POINTER(C.c_longlong)]),
    "sgpu_debug_chain_us": (C.c_int, [C.POINTER(C.c_double)]),
    "sgpu_debug_exchange_mode": (C.c_int, [_VP, _PI]),
    "sgpu_debug_device_info": (C.c_int, [C.c_char_p, C.c_int]),
    "sgpu_debug_allow_local_only": (C.c_int, [_VP, C.c_int]),
    "sgpu_debug_init_host_transport": (C.c_int, [C.c_int, C.c_int, C.c_int, _VP, _VP, _VP]),
    "sgpu_block_pack": (C.c_int, [_VP, _VP, C.c_size_t, C.c_int]),
    "sgpu_block_unpack": (C.c_int, [_VP, _VP, C.c_size_t, C.c_int]),
    "sgpu_op_set_block_lanes": (C.c_int, [_VP, C.c_int]),
    "sgpu_op_get_block_lanes": (C.c_int, [_VP, _PI]),
    "sgpu_spmv_block": (C.c_int, [_VP, _VP, _VP, C.c_int]),
    "sgpu_residual_block": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int]),
    "sgpu_jacobi_block": (C.c_int, [_VP, C.c_int, C.c_double, _VP, _VP, C.c_int]),
    "sgpu_chebyshev_block": (C.c_int, [_VP, C.c_int, C.c_double, _VP, _VP, C.c_int]),
    "sgpu_prolong_correct_block": (C.c_int, [_VP, _VP, _VP, C.c_int]),
    "sgpu_vcycle_block": (C.c_int, [_VP, _VP, _VP, C.c_int]),
    "sgpu_solve_pCG_block": (C.c_int, [_VP, _VP, _VP, C.c_int, _PI, _PD, C.c_int]),
    "sgpu_debug_time_block": (C.c_int, [_VP, C.c_int, _VP, _VP, _VP, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "sgpu_debug_time_vcycle": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "sgpu_debug_block_dot": (C.c_int, [_VP, _VP, _VP, C.c_size_t, C.c_int, C.c_uint, _VP]),
    "sgpu_debug_block_pcg_update": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, C.c_int, C.c_uint, _VP]),
    "sgpu_debug_block_pcg_direction": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_size_t, C.c_int, C.c_uint]),
    "sgpu_solve_FGMRES": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, _PI, _PD, C.c_int, _PD]),
    "sgpu_debug_gs_dots": (C.c_int, [_VP, C.c_size_t, C.c_int, _VP, C.c_size_t, _PD]),
    "sgpu_debug_gs_update": (C.c_int, [_VP, C.c_size_t, C.c_int, _PD, _VP, C.c_size_t, _PD]),
    "sgpu_debug_time_gs": (C.c_int, [C.c_int, _VP, C.c_size_t, C.c_int, _VP, C.c_size_t, C.c_int, C.POINTER(C.c_float)]),
    "sgpu_eigs_LOBPCG": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _PD, _PD, _PI, _PD, C.c_int]),
    "sgpu_eigs_LOBPCG_gen": (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _PD, _PD, _PI, _PD, C.c_int]),
    "sgpu_eigs_LOBPCG_locked": (C.c_int, [_VP, _VP, _VP, _VP, C.c_size_t, C.c_int, _VP, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _PD, _PD,
                                          _PI, _PD, C.c_int, _PI]),
    "sgpu_eigs_LOBPCG_many": (C.c_int, [_VP, _VP, _VP, C.c_size_t, C.c_int, C.c_int, C.c_int, _VP, C.c_int, C.c_double, C.c_int, _PD, _PD, _PI, _PI,
                                        _PI]),
    "sgpu_debug_lock_gram": (C.c_int, [_VP, _VP, C.c_size_t, C.c_int, _VP, C.c_size_t, C.c_int, _VP]),
    "sgpu_debug_lock_project": (C.c_int, [_VP, C.c_size_t, _VP, C.c_int, _VP, C.c_size_t, C.c_int]),
    "sgpu_debug_block_refill": (C.c_int, [_VP, C.c_size_t, C.c_int, C.c_int, C.c_uint]),
    "sgpu_debug_time_lock": (C.c_int, [_VP, C.c_int, _VP, C.c_size_t, C.c_int, _VP, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "sgpu_debug_geig_residual": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_size_t, C.c_int, _VP, _VP]),
    "sgpu_debug_time_geig": (C.c_int, [_VP, _VP, _VP, _VP, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "sgpu_debug_block_gram": (C.c_int, [_VP, _VP, _VP, C.c_size_t, C.c_int, _VP]),
    "sgpu_debug_block_mix": (C.c_int, [C.c_int, C.c_int, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t]),
    "sgpu_debug_eig_residual": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_size_t, C.c_int, _VP]),
    "sgpu_debug_eig_stop": (C.c_int, [_VP, C.c_int, C.c_int]),
    "sgpu_debug_eig_vector": (C.c_int, [_VP, C.c_int, C.c_int, _VP]),
    "sgpu_debug_time_eig": (C.c_int, [_VP, C.c_int, C.c_int, _VP, _VP, _VP, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "sgpu_time_kernel": (C.c_int, [_VP, C.c_int, _VP, _VP, _VP, C.c_int, C.POINTER(C.c_float)]),
    "sgpu_algorithmic_bytes": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_int64)]),
}

_lib = None


def lib():
    """Load libsaena_amd.so (built in-tree by __graft_entry__.build()); raise if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SgpuError(f"{LIB_PATH} is missing: build the HIP extension first "
                            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)          # AttributeError if the ABI lost a symbol
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(status):
    if status != 0:
        msg = lib().sgpu_last_error().decode(errors="replace")
        raise SgpuError(f"libsaena_amd status {status}: {msg}")


_initialised = False


_transport_keep = None


def init_host_transport(device, dist):
    """sgpu_debug_init_host_transport over a torch.distributed group that moves CPU tensors (gloo): this process is
    rank dist.get_rank() of dist.get_world_size(); halos and scalar reductions are routed through the host.  For
    validating the multi-rank code with several processes on ONE card (RCCL needs one device per rank)."""
    global _initialised, _transport_keep
    import torch
    rank, world = dist.get_rank(), dist.get_world_size()
    XF = C.CFUNCTYPE(C.c_int, _VP, _VP, _PI, _PI, C.c_int, _VP, _PI, _PI, C.c_int, C.c_int)
    AF = C.CFUNCTYPE(C.c_int, _VP, _PD, C.c_int)

    def view(ptr, nbytes):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(nbytes,)) if nbytes else np.zeros(0, np.uint8)

    def exchange(user, send, srank, scount, nsend, recv, rrank, rcount, nrecv, eb):
        try:
            reqs, outs, keep = [], [], []
            so = 0
            for i in range(nsend):
                n = scount[i] * eb
                t = torch.from_numpy(view(send + so if send else None, n).copy())
                keep.append(t)
                reqs.append(dist.isend(t, srank[i]))
                so += n
            ro = 0
            for i in range(nrecv):
                n = rcount[i] * eb
                t = torch.empty(n, dtype=torch.uint8)
                outs.append((ro, n, t))
                reqs.append(dist.irecv(t, rrank[i]))
                ro += n
            for rq in reqs:
                rq.wait()
            for ro, n, t in outs:
                if n:
                    view(recv + ro, n)[:] = t.numpy()
            return 0
        except Exception as e:      # pragma: no cover
            print("host transport exchange failed:", e)
            return 1

    def allreduce(user, v, n):
        try:
            a = np.ctypeslib.as_array(v, shape=(n,))
            t = torch.from_numpy(a.copy())
            dist.all_reduce(t)
            a[:] = t.numpy()
            return 0
        except Exception as e:      # pragma: no cover
            print("host transport allreduce failed:", e)
            return 1
    xf, af = XF(exchange), AF(allreduce)
    _transport_keep = (xf, af)
    check(lib().sgpu_debug_init_host_transport(int(device), rank, world, C.cast(xf, _VP), C.cast(af, _VP), None))
    _initialised = True


def init(device=0, rank=0, nranks=1, unique_id=None):
    """sgpu_init; raises SgpuError when no MI355X is visible."""
    global _initialised
    if _initialised:
        return
    buf = None
    if unique_id is not None:
        buf = C.create_string_buffer(bytes(unique_id), 128)
    check(lib().sgpu_init(device, rank, nranks, buf))
    _initialised = True


def finalize():
    global _initialised
    if _initialised:
        check(lib().sgpu_finalize())
        _initialised = False


def get_unique_id():
    buf = C.create_string_buffer(128)
    check(lib().sgpu_get_unique_id(buf))
    return buf.raw


class DeviceVector:
    """A row slice in HBM (raw device pointer + length)."""

    def __init__(self, n, host=None):
        self.n = int(n)
        p = _VP()
        check(lib().sgpu_vec_alloc(C.byref(p), self.n))
        self.ptr = p
        if host is not None:
            self.upload(host)

    def upload(self, host):
        host = np.ascontiguousarray(host, np.float64)
        assert host.size == self.n
        check(lib().sgpu_vec_upload(self.ptr, host.ctypes.data, self.n))
        return self

    def download(self):
        out = np.empty(self.n, np.float64)
        check(lib().sgpu_vec_download(out.ctypes.data, self.ptr, self.n))
        return out

    def fill(self, a):
        check(lib().sgpu_vec_fill(self.ptr, float(a), self.n))
        return self

    def free(self):
        if self.ptr:
            lib().sgpu_vec_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            if _initialised:
                self.free()
        except Exception:
            pass


class BlockVector:
    """K columns over n rows in HBM, interleaved (X[i*K + j]); host arrays are (n, K), column j = host[:, j].  The library
    converts between its layout and the column-major one callers use (sgpu_block_pack / sgpu_block_unpack)."""

    def __init__(self, n, K, host=None):
        self.n, self.K = int(n), int(K)
        p = _VP()
        check(lib().sgpu_vec_alloc(C.byref(p), self.n * self.K))
        self.ptr = p
        if host is not None:
            self.upload(host)

    def upload(self, host):
        host = np.asarray(host, np.float64)
        assert host.shape == (self.n, self.K), host.shape
        cm = DeviceVector(self.n * self.K, np.asfortranarray(host).ravel(order="F"))     # column-major n x K
        check(lib().sgpu_block_pack(cm.ptr, self.ptr, self.n, self.K))
        check(lib().sgpu_device_sync())
        cm.free()
        return self

    def download(self):
        cm = DeviceVector(self.n * self.K)
        check(lib().sgpu_block_unpack(self.ptr, cm.ptr, self.n, self.K))
        out = cm.download().reshape((self.n, self.K), order="F")
        cm.free()
        return out

    def free(self):
        if self.ptr:
            lib().sgpu_vec_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            if _initialised:
                self.free()
        except Exception:
            pass


def _ai(a):
    return np.ascontiguousarray(a, np.int32)


def _ad(a):
    return np.ascontiguousarray(a, np.float64)


EXCHANGE_MODES = ("none", "host-transport", "one-stream", "kernel-flags", "value-ops", "events")


class Operator:
    """sgpu_op built from one rank's arrays in the reference's storage layout."""

    def __init__(self, *, M, N_local, col_offset, nnzPerRow_local, col_local, val_local,
                 nnzPerCol_remote=(), row_remote=(), val_remote=(),
                 recvProcRank=(), recvProcCount=(), sendProcRank=(), sendProcCount=(), vIndex=(),
                 inv_diag=None, halo_fp32=False):
        keep = self._keep = {}
        keep["npr"], keep["col"], keep["val"] = _ai(nnzPerRow_local), _ai(col_local), _ad(val_local)
        keep["npc"], keep["rr"], keep["rv"] = _ai(nnzPerCol_remote), _ai(row_remote), _ad(val_remote)
        keep["rpr"], keep["rpc"] = _ai(recvProcRank), _ai(recvProcCount)
        keep["spr"], keep["spc"], keep["vi"] = _ai(sendProcRank), _ai(sendProcCount), _ai(vIndex)
        keep["inv"] = None if inv_diag is None else _ad(inv_diag)
        d = OpDesc()
        d.M, d.N_local, d.col_offset = int(M), int(N_local), int(col_offset)
        d.nnz_l_local = len(keep["col"])
        d.nnzPerRow_local = keep["npr"].ctypes.data_as(_PI)
        d.col_local = keep["col"].ctypes.data_as(_PI)
        d.val_local = keep["val"].ctypes.data_as(_PD)
        d.nnz_l_remote = len(keep["rr"])
        d.col_remote_size = len(keep["npc"])
        d.nnzPerCol_remote = keep["npc"].ctypes.data_as(_PI)
        d.row_remote = keep["rr"].ctypes.data_as(_PI)
        d.val_remote = keep["rv"].ctypes.data_as(_PD)
        d.numRecvProc, d.numSendProc = len(keep["rpr"]), len(keep["spr"])
        d.recvProcRank = keep["rpr"].ctypes.data_as(_PI)
        d.recvProcCount = keep["rpc"].ctypes.data_as(_PI)
        d.sendProcRank = keep["spr"].ctypes.data_as(_PI)
        d.sendProcCount = keep["spc"].ctypes.data_as(_PI)
        d.vIndexSize = len(keep["vi"])
        d.vIndex = keep["vi"].ctypes.data_as(_PI)
        d.inv_diag = keep["inv"].ctypes.data_as(_PD) if keep["inv"] is not None else None
        d.halo_fp32 = 1 if halo_fp32 else 0
        h = _VP()
        check(lib().sgpu_op_create(C.byref(d), C.byref(h)))
        self.h = h
        self.M, self.N_local = int(M), int(N_local)
        self._keep = None      # the library copied everything

    def info(self):
        M, N, nb, ln = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        nl, nr = C.c_long(), C.c_long()
        check(lib().sgpu_op_info(self.h, C.byref(M), C.byref(N), C.byref(nl), C.byref(nr), C.byref(nb), C.byref(ln)))
        return dict(M=M.value, N_local=N.value, nnz_local=nl.value, nnz_remote=nr.value, row_blocks=nb.value,
                    lanes_per_row=ln.value)

    def set_lanes_per_row(self, lanes):
        check(lib().sgpu_op_set_lanes_per_row(self.h, int(lanes)))

    def block_plan(self, big=0):
        """spread of work over the row blocks of the tile kernels' plan (sgpu_debug_block_plan)"""
        o = (C.c_long * 8)()
        check(lib().sgpu_debug_block_plan(self.h, int(big), o))
        k = ("blocks", "min_nnz_per_block", "max_nnz_per_block", "nnz", "min_rows_per_block", "max_rows_per_block", "long_rows", "longest_row")
        return dict(zip(k, (int(x) for x in o)))

    def xlds_plan(self):
        """the x-in-LDS plan of variants 10 / 12 / 16 (sgpu_debug_block_plan, big = 2)"""
        o = (C.c_long * 8)()
        check(lib().sgpu_debug_block_plan(self.h, 2, o))
        return dict(zip(("chunks", "windows", "window_columns", "sums_in_lds", "max_rows_per_chunk"), (int(x) for x in o)))

    def variant(self):
        v, name = C.c_int(), C.c_char_p()
        check(lib().sgpu_op_get_variant(self.h, C.byref(v), C.byref(name)))
        return v.value, name.value.decode()

    def autotune(self):
        check(lib().sgpu_op_autotune(self.h))

    def set_variant(self, variant):
        check(lib().sgpu_op_set_variant(self.h, int(variant)))

    def set_x_windows(self, rows_per_workgroup):
        """x-window launch mode of variant 17: 256 / 512 / 1024 rows per workgroup, 0 = direct gathers; raises where it is refused"""
        check(lib().sgpu_op_set_x_windows(self.h, int(rows_per_workgroup)))

    def x_windows(self):
        """rows per workgroup of the x-window mode in use, 0 = direct gathers"""
        v = C.c_int()
        check(lib().sgpu_op_get_x_windows(self.h, C.byref(v)))
        return v.value

    def x_window_kernel(self):
        """which kernel the x-window mode runs (of the last launch in the mode, once there was one): 0 k_vidxw or the mode is off,
        1 k_vidxw_fast with its dictionaries in LDS, 2 k_vidxw_fast with dictionaries of at most two values in scalar registers"""
        v = C.c_int()
        check(lib().sgpu_op_get_x_window_kernel(self.h, C.byref(v)))
        return v.value

    def x_window_code_width(self):
        """bits per entry of the code stream variant 17 reads (of the last launch in the mode, once there was one): 8, or 1 where
        k_vidxw_fast reads the codes of scalar dictionaries packed to one bit per entry; 0: another variant"""
        v = C.c_int()
        check(lib().sgpu_op_get_x_window_code_width(self.h, C.byref(v)))
        return v.value

    def x_window_row_format(self):
        """how k_vidxw_fast reads its rows (of the last launch in the mode, once there was one): 1 as lane masks in scalar registers,
        0 through the pattern table (or the mode is off, or another variant)"""
        v = C.c_int()
        check(lib().sgpu_op_get_x_window_row_format(self.h, C.byref(v)))
        return v.value

    def exchange_mode(self):
        """how the next scalar apply orders its exchange (sgpu_debug_exchange_mode): an index into EXCHANGE_MODES"""
        v = C.c_int()
        check(lib().sgpu_debug_exchange_mode(self.h, C.byref(v)))
        return EXCHANGE_MODES[v.value]

    def storage_mask(self):
        """bit mask of the local part's storage groups that hold device memory (sgpu_debug_op_storage; bit order: STORAGE_GROUPS)"""
        m, b = C.c_uint(), C.c_longlong()
        check(lib().sgpu_debug_op_storage(self.h, C.byref(m), C.byref(b)))
        return m.value

    def spmv(self, v, w):
        check(lib().sgpu_spmv(self.h, v.ptr, w.ptr))

    def residual(self, u, rhs, res):
        check(lib().sgpu_residual(self.h, u.ptr, rhs.ptr, res.ptr))

    def residual_negative(self, u, rhs, res):
        check(lib().sgpu_residual_negative(self.h, u.ptr, rhs.ptr, res.ptr))

    def residual_multiply(self, u, rhs, res, w, c):
        check(lib().sgpu_residual_multiply(self.h, u.ptr, rhs.ptr, res.ptr, w.ptr, float(c)))

    def jacobi(self, it, u, rhs, omega=0.0):
        check(lib().sgpu_jacobi(self.h, int(it), float(omega), u.ptr, rhs.ptr))

    def chebyshev(self, it, eig_max, u, rhs):
        check(lib().sgpu_chebyshev(self.h, int(it), float(eig_max), u.ptr, rhs.ptr))

    def prolong_correct(self, e_coarse, u):
        check(lib().sgpu_prolong_correct(self.h, e_coarse.ptr, u.ptr))

    def eig_max(self, steps=20):
        """the Chebyshev smoother's eig_max of this operator, estimated on the device (sgpu_op_eig_max): the host setup's Lanczos
        recurrence through the operator's current SpMV form; steps in 1..64, 0 = the setup's 20"""
        v = C.c_double()
        check(lib().sgpu_op_eig_max(self.h, int(steps), C.byref(v)))
        return v.value

    # block vectors (BlockVector): K right-hand sides through one pass over the operator
    def set_block_lanes(self, lanes):
        check(lib().sgpu_op_set_block_lanes(self.h, int(lanes)))

    def block_lanes(self):
        v = C.c_int()
        check(lib().sgpu_op_get_block_lanes(self.h, C.byref(v)))
        return v.value

    def spmv_block(self, X, Y):
        check(lib().sgpu_spmv_block(self.h, X.ptr, Y.ptr, X.K))

    def residual_block(self, U, RHS, RES):
        check(lib().sgpu_residual_block(self.h, U.ptr, RHS.ptr, RES.ptr, U.K))

    def jacobi_block(self, it, U, RHS, omega=0.0):
        check(lib().sgpu_jacobi_block(self.h, int(it), float(omega), U.ptr, RHS.ptr, U.K))

    def chebyshev_block(self, it, eig_max, U, RHS):
        check(lib().sgpu_chebyshev_block(self.h, int(it), float(eig_max), U.ptr, RHS.ptr, U.K))

    def prolong_correct_block(self, E_coarse, U):
        check(lib().sgpu_prolong_correct_block(self.h, E_coarse.ptr, U.ptr, U.K))

    def time_block(self, kind, X, RHS, Y, reps):
        """ms per launch of the block kernel, timed inside the library like time_kernel (kind 0: product, 1: Jacobi sweep X -> Y)"""
        ms = C.c_float()
        check(lib().sgpu_debug_time_block(self.h, kind, X.ptr, RHS.ptr if RHS is not None else None, Y.ptr, X.K, reps, C.byref(ms)))
        return ms.value

    def debug_gather_probe(self, mode, x, reps=20):
        ms = C.c_float()
        check(lib().sgpu_debug_gather_probe(self.h, mode, x.ptr, reps, C.byref(ms)))
        return ms.value

    def debug_pack(self, v, n_send):
        out = np.empty(n_send)
        check(lib().sgpu_debug_pack(self.h, v.ptr, out.ctypes.data_as(_PD)))
        return out

    def debug_allow_local_only(self, allow=True):
        check(lib().sgpu_debug_allow_local_only(self.h, 1 if allow else 0))

    def debug_inject_halo(self, recv):
        recv = _ad(recv)
        check(lib().sgpu_debug_inject_halo(self.h, recv.ctypes.data_as(_PD)))

    def debug_pack_block(self, X, n_send):
        """-> (n_send, K): the block send buffer after the pack kernel, row t = the K columns of X at vIndex[t]"""
        out = np.empty((n_send, X.K))
        check(lib().sgpu_debug_pack_block(self.h, X.ptr, X.K, out.ctypes.data_as(_PD)))
        return out

    def debug_inject_halo_block(self, recv):
        """recv: (recvSize, K), row p = the K columns at halo position p"""
        recv = _ad(recv)
        check(lib().sgpu_debug_inject_halo_block(self.h, recv.shape[1], recv.ctypes.data_as(_PD)))

    def spmv_host(self, v):
        v = _ad(v)
        w = np.empty(self.M)
        check(lib().sgpu_spmv_host(self.h, v.ctypes.data_as(_PD), w.ctypes.data_as(_PD)))
        return w

    def algorithmic_bytes(self, kind=0):
        b = C.c_int64()
        check(lib().sgpu_algorithmic_bytes(self.h, kind, C.byref(b)))
        return b.value

    def time_kernel(self, kind, x, rhs, y, reps):
        ms = C.c_float()
        check(lib().sgpu_time_kernel(self.h, kind, x.ptr, rhs.ptr if rhs is not None else None, y.ptr, reps, C.byref(ms)))
        return ms.value

    def destroy(self):
        if self.h:
            lib().sgpu_op_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if _initialised:
                self.destroy()
        except Exception:
            pass


def coarse_solver_code(name):
    """sgpu_amg_params.coarse_solver of a name: "direct" 1, "device_cg" 2, anything else ("CG", "cg") 0"""
    return {"direct": 1, "device_cg": 2}.get(name, 0)


def null_space_code(name):
    """sgpu_amg_create_null_space's null_space of a name: "none" 0, "constant" 1; an int is passed through"""
    if isinstance(name, str):
        if name not in ("none", "constant"):
            raise ValueError(f'null_space is "none" or "constant", not {name!r}')
        return {"none": 0, "constant": 1}[name]
    return int(name)


class Amg:
    """sgpu_amg over Operators A[l], P[l], R[l]."""

    def __init__(self, A, P, R, eig_max=None, pre=3, post=3, smoother="jacobi", max_iter=100, tol=1e-8, use_graph=True, coarse_solver="direct",
                 cg_max_iter=150, cg_tol=1e-12, null_space=None):
        """null_space: None / "none" -> sgpu_amg_create, as ever; "constant" -> sgpu_amg_create_null_space(..., 1, ...): the operators
        annihilate constants, the solvers solve A u = rhs - mean(rhs) and return the solution of zero mean; an int is passed through"""
        self.A, self.P, self.R = list(A), list(P), list(R)
        n = len(A)
        prm = AmgParams()
        check(lib().sgpu_amg_default_params(C.byref(prm)))
        prm.preSmooth, prm.postSmooth = pre, post
        prm.smoother = 0 if smoother == "jacobi" else 1
        prm.solver_max_iter, prm.solver_tol = max_iter, tol
        prm.use_graph = 1 if use_graph else 0
        prm.coarse_solver = coarse_solver_code(coarse_solver)
        prm.CG_coarsest_max_iter, prm.CG_coarsest_tol = int(cg_max_iter), float(cg_tol)
        HA = (_VP * n)(*[a.h for a in A])
        HP = (_VP * n)(*([p.h for p in P] + [None] * (n - len(P))))
        HR = (_VP * n)(*([r.h for r in R] + [None] * (n - len(R))))
        eig = None
        if eig_max is not None:
            eig = _ad(eig_max)
        h = _VP()
        pe = eig.ctypes.data_as(_PD) if eig is not None else None
        if null_space is None:
            check(lib().sgpu_amg_create(n, HA, HP, HR, pe, C.byref(prm), C.byref(h)))
        else:
            check(lib().sgpu_amg_create_null_space(n, HA, HP, HR, pe, C.byref(prm), null_space_code(null_space), C.byref(h)))
        self.h = h

    @property
    def null_space(self):
        """sgpu_amg_get_null_space: 0 none, 1 constants"""
        k = C.c_int(-1)
        check(lib().sgpu_amg_get_null_space(self.h, C.byref(k)))
        return k.value

    def vcycle(self, u, rhs):
        check(lib().sgpu_vcycle(self.h, u.ptr, rhs.ptr))

    def coarsest_solve(self, u, rhs):
        it = C.c_int()
        check(lib().sgpu_coarsest_solve(self.h, u.ptr, rhs.ptr, C.byref(it)))
        return it.value

    def _solve(self, fn, u, rhs, cap=256):
        it = C.c_int()
        hist = np.full(cap, np.nan)
        st = fn(self.h, u.ptr, rhs.ptr, C.byref(it), hist.ctypes.data_as(_PD), cap)
        if st not in (0, -6):
            check(st)
        return it.value, hist[:min(it.value + 1, cap)], st == 0     # entries 0..iters as written: a non-finite one stays visible

    def solve(self, u, rhs):
        return self._solve(lib().sgpu_solve, u, rhs)

    def solve_pCG(self, u, rhs):
        return self._solve(lib().sgpu_solve_pCG, u, rhs)

    def solve_CG(self, u, rhs):
        return self._solve(lib().sgpu_solve_CG, u, rhs, cap=2048)

    def solve_smoother(self, u, rhs):
        return self._solve(lib().sgpu_solve_smoother, u, rhs, cap=2048)

    def solve_fgmres(self, u, rhs, restart=30, precond=True, cap=4096):
        """-> (iters, history, converged, true_res): sgpu_solve_FGMRES; history[0] = ||r_0||, history[k] the Givens estimate after inner
        iteration k, true_res the last recomputed ||rhs - A u||"""
        it, tr = C.c_int(), C.c_double()
        hist = np.full(cap, np.nan)
        st = lib().sgpu_solve_FGMRES(self.h, u.ptr, rhs.ptr, int(restart), 1 if precond else 0, C.byref(it), hist.ctypes.data_as(_PD), cap, C.byref(tr))
        if st not in (0, -6):
            check(st)
        return it.value, hist[~np.isnan(hist)], st == 0, tr.value

    def vcycle_block(self, U, RHS):
        check(lib().sgpu_vcycle_block(self.h, U.ptr, RHS.ptr, U.K))

    def time_vcycle(self, u, rhs, reps):
        """ms per V-cycle, `reps` of them back to back inside the library; u / rhs: DeviceVectors (scalar) or BlockVectors"""
        ms = C.c_float()
        check(lib().sgpu_debug_time_vcycle(self.h, u.ptr, rhs.ptr, getattr(u, "K", 0), reps, C.byref(ms)))
        return ms.value

    def time_dcg_matvec(self, x, y, reps):
        """ms per launch of the device coarsest CG's product kernel on the coarsest operator (sgpu_debug_dcg_matvec_time)"""
        ms = C.c_float()
        check(lib().sgpu_debug_dcg_matvec_time(self.h, x.ptr, y.ptr, int(reps), C.byref(ms)))
        return ms.value

    def solve_pCG_block(self, U, RHS, cap=256):
        """-> (iters[K], [history of column j], converged): sgpu_solve_pCG_block"""
        K = U.K
        it = (C.c_int * K)()
        hist = np.full((K, cap), np.nan)
        st = lib().sgpu_solve_pCG_block(self.h, U.ptr, RHS.ptr, K, it, hist.ctypes.data_as(_PD), cap)
        if st not in (0, -6):
            check(st)
        return [int(v) for v in it], [h[:min(int(k) + 1, cap)] for h, k in zip(hist, it)], st == 0

    # the block dot and the block pCG updates on the caller's device vectors (sgpu_debug_block_*): n rows of K interleaved columns
    def debug_block_dot(self, X, Y, n, K, active, out):
        check(lib().sgpu_debug_block_dot(self.h, X.ptr, Y.ptr, int(n), int(K), int(active), out.ptr))

    def debug_block_pcg_update(self, num, den, P, H, U, R, n, K, active, rr):
        check(lib().sgpu_debug_block_pcg_update(self.h, num.ptr, den.ptr, P.ptr, H.ptr, U.ptr, R.ptr, int(n), int(K), int(active), rr.ptr))

    def debug_block_pcg_direction(self, num, den, Z, P, n, K, active):
        check(lib().sgpu_debug_block_pcg_direction(self.h, num.ptr, den.ptr, Z.ptr, P.ptr, int(n), int(K), int(active)))

    def lobpcg(self, X, nev, max_iter=100, tol=1e-8, precond=True, cap=512, B=None):
        """sgpu_eigs_LOBPCG on the block vector X (anything with .ptr and .K; start vectors in, eigenvectors out); with B (an
        Operator, or anything with .h) sgpu_eigs_LOBPCG_gen: A x = lambda B x, X B-orthonormal on return
        -> (lambda[K], res[K], iterations, [history of column j], converged)"""
        K = X.K
        lam, res, it = np.full(K, np.nan), np.full(K, np.nan), C.c_int()
        hist = np.full((K, cap), np.nan)
        if B is None:
            st = lib().sgpu_eigs_LOBPCG(self.h, X.ptr, K, int(nev), int(max_iter), float(tol), 1 if precond else 0, lam.ctypes.data_as(_PD),
                                        res.ctypes.data_as(_PD), C.byref(it), hist.ctypes.data_as(_PD), cap)
        else:
            st = lib().sgpu_eigs_LOBPCG_gen(self.h, B.h, X.ptr, K, int(nev), int(max_iter), float(tol), 1 if precond else 0,
                                            lam.ctypes.data_as(_PD), res.ctypes.data_as(_PD), C.byref(it), hist.ctypes.data_as(_PD), cap)
        if st not in (0, -6):
            check(st)
        return lam, res, it.value, [h[~np.isnan(h)] for h in hist], st == 0

    def lobpcg_locked(self, X, nev, Q=None, ld=None, nlocked=0, BQ=None, B=None, max_iter=100, tol=1e-8, precond=True, cap=512):
        """sgpu_eigs_LOBPCG_locked: lobpcg() constrained to the B-orthogonal complement of the first nlocked columns of Q (anything
        with .ptr: column-major on the device, column l at l * ld; BQ = B Q the same way, read when B is given)
        -> (lambda[K], res[K], iterations, [history of column j], converged, leading)"""
        K = X.K
        lam, res, it, lead = np.full(K, np.nan), np.full(K, np.nan), C.c_int(), C.c_int()
        hist = np.full((K, cap), np.nan)
        st = lib().sgpu_eigs_LOBPCG_locked(self.h, B.h if B is not None else None, Q.ptr if Q is not None else None,
                                           BQ.ptr if BQ is not None else None, int(ld), int(nlocked), X.ptr, K, int(nev), int(max_iter), float(tol),
                                           1 if precond else 0, lam.ctypes.data_as(_PD), res.ctypes.data_as(_PD), C.byref(it),
                                           hist.ctypes.data_as(_PD), cap, C.byref(lead))
        if st not in (0, -6):
            check(st)
        return lam, res, it.value, [h[~np.isnan(h)] for h in hist], st == 0, lead.value

    def lobpcg_many(self, n, nev, K, sweep_nev=0, X0=None, B=None, max_iter=400, tol=1e-8, precond=True, ld=None, nan_padding=False):
        """sgpu_eigs_LOBPCG_many: the nev <= 64 smallest eigenpairs of the level-0 operator of n rows (of A x = lambda B x with B) by
        sweeps of the locked block solve on K columns.  X0: a block vector of K start columns (anything with .ptr), or None for generated ones
        -> (lambda[nlocked], res[nlocked], Q (n, nlocked) host array, total iterations, sweeps, converged)"""
        n = int(n)
        ld = int(ld) if ld is not None else n + (n & 1)
        dQ = DeviceVector(max(1, nev * ld))
        if nan_padding:
            dQ.fill(float("nan"))
        lam, res = np.full(nev, np.nan), np.full(nev, np.nan)
        it, nl, sw = C.c_int(), C.c_int(), C.c_int()
        st = lib().sgpu_eigs_LOBPCG_many(self.h, B.h if B is not None else None, dQ.ptr, ld, int(nev), int(K), int(sweep_nev),
                                         X0.ptr if X0 is not None else None, int(max_iter), float(tol), 1 if precond else 0,
                                         lam.ctypes.data_as(_PD), res.ctypes.data_as(_PD), C.byref(it), C.byref(nl), C.byref(sw))
        if st not in (0, -6):
            check(st)
        L = nl.value
        Q = dQ.download().reshape(nev, ld)[:L, :n].T.copy() if nev * ld else np.zeros((n, 0))
        return lam[:L], res[:L], Q, it.value, sw.value, st == 0

    # the launch helpers of hard locking on the caller's device arrays (sgpu_debug_lock_gram / _lock_project / _block_refill)
    def debug_lock_gram(self, Z, ld, L, Y, n, K, out):
        check(lib().sgpu_debug_lock_gram(self.h, Z.ptr, int(ld), int(L), Y.ptr, int(n), int(K), out.ptr))

    def time_lock(self, kind, Q, ld, L, Y, n, K, reps):
        ms = C.c_float()
        check(lib().sgpu_debug_time_lock(self.h, int(kind), Q.ptr, int(ld), int(L), Y.ptr, int(n), int(K), int(reps), C.byref(ms)))
        return ms.value

    # the LOBPCG launch helpers on the caller's device vectors (sgpu_debug_block_gram / _block_mix / _eig_residual)
    def debug_block_gram(self, X, Y, n, K, out):
        check(lib().sgpu_debug_block_gram(self.h, X.ptr, Y.ptr, int(n), int(K), out.ptr))

    def debug_eig_residual(self, AX, X, lam, R, n, K, rr):
        check(lib().sgpu_debug_eig_residual(self.h, AX.ptr, X.ptr, lam.ptr, R.ptr, int(n), int(K), rr.ptr))

    def debug_geig_residual(self, AX, BX, lam, R, n, K, rr, bb):
        check(lib().sgpu_debug_geig_residual(self.h, AX.ptr, BX.ptr, lam.ptr, R.ptr, int(n), int(K), rr.ptr, bb.ptr))

    def time_geig(self, AX, BX, R, n, K, reps):
        ms = C.c_float()
        check(lib().sgpu_debug_time_geig(self.h, AX.ptr, BX.ptr, R.ptr, int(n), int(K), int(reps), C.byref(ms)))
        return ms.value

    def debug_eig_stop(self, K, iteration):
        check(lib().sgpu_debug_eig_stop(self.h, int(K), int(iteration)))

    def debug_eig_vector(self, K, which, dst):
        check(lib().sgpu_debug_eig_vector(self.h, int(K), int(which), dst.ptr))

    def time_eig(self, kind, ns, X, Y, Out, n, K, reps):
        ms = C.c_float()
        check(lib().sgpu_debug_time_eig(self.h, int(kind), int(ns), X.ptr, Y.ptr, Out.ptr, int(n), int(K), int(reps), C.byref(ms)))
        return ms.value

    def set_solve_params(self, max_iter, tol, smoother, pre, post):
        check(lib().sgpu_amg_set_solve_params(self.h, int(max_iter), float(tol), 0 if smoother == "jacobi" else 1, int(pre), int(post)))

    def set_operator(self, level, op, eig_max=0.0):
        """sgpu_amg_set_operator: `op` replaces A of `level` (same size, one rank); every captured graph of the hierarchy is dropped.
        The operator it replaces stays alive and the caller's: destroy it after this call.  Returns that operator."""
        check(lib().sgpu_amg_set_operator(self.h, int(level), op.h, float(eig_max)))
        old, self.A[level] = self.A[level], op
        return old

    def profile_matvecs(self, iters=5):
        us = np.zeros(len(self.A))
        check(lib().sgpu_amg_profile_matvecs(self.h, int(iters), us.ctypes.data_as(_PD)))
        return us

    def destroy(self):
        if self.h:
            lib().sgpu_amg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if _initialised:
                self.destroy()
        except Exception:
            pass


def stream_ceiling(read_bytes, write_bytes, reps=20):
    """-> (microseconds, mode name, bytes moved) of the fastest pure streaming kernel over this byte mix (sgpu_debug_stream_ceiling)"""
    us, mode, moved = C.c_float(), C.c_int(), C.c_size_t()
    check(lib().sgpu_debug_stream_ceiling(int(read_bytes), int(write_bytes), int(reps), C.byref(us), C.byref(mode), C.byref(moved)))
    return us.value, ("plain loads and stores", "non-temporal loads", "non-temporal stores", "non-temporal loads and stores")[mode.value], moved.value


def device_info():
    """one line about the context's device, plus the amdgpu partition modes where sysfs shows them"""
    buf = C.create_string_buffer(512)
    check(lib().sgpu_debug_device_info(buf, 512))
    line = buf.value.decode()
    import glob
    for key in ("current_compute_partition", "current_memory_partition"):
        vals = set()
        for f in glob.glob(f"/sys/class/drm/card*/device/{key}"):
            try:
                vals.add(open(f).read().strip())
            except OSError:
                pass
        if vals:
            line += f", {key.replace('current_', '')} {'/'.join(sorted(vals))}"
    return line


def chain_us():
    """the exchange chain sgpu_init measured on the communicator, microseconds (0 without one)"""
    v = C.c_double()
    check(lib().sgpu_debug_chain_us(C.byref(v)))
    return v.value


def gs_dots(V, ld, ncols, w, n):
    """-> h[ncols] = V[:,c] . w through the FGMRES launch helper (sgpu_debug_gs_dots); V, w: DeviceVectors (or anything with .ptr)"""
    out = np.empty(int(ncols))
    check(lib().sgpu_debug_gs_dots(V.ptr, int(ld), int(ncols), w.ptr, int(n), out.ctypes.data_as(_PD)))
    return out


def gs_update(V, ld, ncols, h, w, n, norm=False):
    """w -= sum_c h[c] V[:,c] on the device (sgpu_debug_gs_update); -> the fused ||w||^2 when norm, else None"""
    h = _ad(h)
    assert h.size == ncols
    nrm = C.c_double()
    check(lib().sgpu_debug_gs_update(V.ptr, int(ld), int(ncols), h.ctypes.data_as(_PD), w.ptr, int(n), C.byref(nrm) if norm else None))
    return nrm.value if norm else None


def time_gs(kind, V, ld, ncols, w, n, reps):
    ms = C.c_float()
    check(lib().sgpu_debug_time_gs(int(kind), V.ptr, int(ld), int(ncols), w.ptr, int(n), int(reps), C.byref(ms)))
    return ms.value


def block_mix(K, sources, coefs, out, n, add=None):
    """out = sum_s sources[s] coefs[s] (+ add) on block vectors of n rows (sgpu_debug_block_mix); 1 to 3 sources, coefs: device, K x K"""
    ns = len(sources)
    assert ns == len(coefs) and 1 <= ns <= 3
    p = []
    for s in range(3):
        p += [sources[s].ptr, coefs[s].ptr] if s < ns else [None, None]
    check(lib().sgpu_debug_block_mix(int(K), ns, *p, add.ptr if add is not None else None, out.ptr, int(n)))


# the storage groups of an operator's local part, in the bit order of sgpu_debug_op_storage
STORAGE_GROUPS = ("csr", "dense", "cc0", "cc1", "cm0", "cm1", "sell_values", "sell_columns", "sellp", "vidx", "xwin256", "xwin512",
                  "xwin1024", "sellp2", "sellpx", "rowt", "xlds_plan", "xlds_columns", "sellx")


def live_bytes():
    """bytes held by all of the library's owned device and pinned arrays in this process (sgpu_debug_op_storage)"""
    m, b = C.c_uint(), C.c_longlong()
    st = lib().sgpu_debug_op_storage(None, C.byref(m), C.byref(b))
    check(st)
    return b.value


def lock_project(K, Q, ld, Cm, L, W, n):
    """W <- W - Q C on a block vector of n rows (sgpu_debug_lock_project); Q: L column-major columns of ld, Cm: device, L x K"""
    check(lib().sgpu_debug_lock_project(Q.ptr, int(ld), Cm.ptr, int(L), W.ptr, int(n), int(K)))


def block_refill(X, n, K, col, counter):
    """column col of the block vector X from the refill generator (sgpu_debug_block_refill)"""
    check(lib().sgpu_debug_block_refill(X.ptr, int(n), int(K), int(col), int(counter)))


def launch_count():
    n = C.c_long()
    check(lib().sgpu_debug_launch_count(C.byref(n)))
    return n.value


def vec_center(x, y=None, want_mean=False):
    """sgpu_vec_center: y = x - mean(x) on DeviceVectors (y None: in place) -> the mean that was subtracted when want_mean, else None"""
    m = C.c_double(float("nan"))
    check(lib().sgpu_vec_center(x.ptr, (x if y is None else y).ptr, x.n, C.byref(m) if want_mean else None))
    return m.value if want_mean else None


def block_center(X, Y=None):
    """sgpu_block_center on BlockVectors (Y None: in place)"""
    check(lib().sgpu_block_center(X.ptr, (X if Y is None else Y).ptr, X.n, X.K))


def dot(x, y):
    out = C.c_double()
    check(lib().sgpu_dot(x.ptr, y.ptr, x.n, C.byref(out)))
    return out.value
