"""The exchanged apply on ONE GPU, held to the forms' contract on a mirror world (run as a subprocess by tests/test_gpu_rccl_mirror.py;
`--torch` imports torch first, the configuration of `bench.py --gpus N`; `--expect MODE` names the ordering the environment selects).

tests/mirror_world.py: rank 0 of the 2-rank operator [[B, C], [C, B]] sends exactly what it receives, so with its peer rewired to itself
it exchanges for real over a 1-rank communicator, and what arrives is x[vIndex].  Every case builds two operators from one descriptor:
one exchanges; the twin gets x[vIndex] injected (through float on the fp32 wire) and runs the same kernels on one stream.
  * every apply (spmv, the residuals, a Jacobi sweep, a Chebyshev step, u -= A e) runs four times back to back on four inputs into
    NaN-filled outputs, an input overwritten with NaN right behind each apply, no host synchronisation in between: all four outputs
    are the twin's bits, under every form of tests/test_gpu_forms.py that takes the operator;
  * the twin meets the forms' contract against mirror_world.apply_plain;
  * Jacobi (4 sweeps) and Chebyshev (3 steps) chains against the 2-rank oracle's rank-0 slice;
  * the block twin (K = 2, 8) and two mirrored hierarchies (V-cycle, solve, pCG) against the one-rank oracle;
  * sgpu_debug_exchange_mode reports the expected ordering on every operator.
One JSON line per case with sha256 digests of every output: the parent holds them equal across orderings."""
import sys

if "--torch" in sys.argv:
    import torch  # noqa: F401

import hashlib
import json
import os
import time

import numpy as np

from oracle import oracle as orc
from saena_amd import capi
from tests import hierarchy, inputs
from tests import mirror_world as mw
from tests import test_gpu_forms as F
from tests.test_gpu_vcycle import TOL_HIST, TOL_VCYCLE

EXPECT = sys.argv[sys.argv.index("--expect") + 1]
NAN = float("nan")
TOL_F32_CHAIN = 1e-6                         # of max |ref|: the fp32 wire rounds the halo of every step (tests/rccl_loopback.py)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(F.bits(a).tobytes())
    return h.hexdigest()


def expected_modes(G, near_threshold=False):
    """the orderings this environment may select for an operator: the dense form with a halo has no interior / boundary split (one
    stream).  near_threshold: hub's 1.26 M local entries sit where sgpu_op_create's one-stream threshold (1 M entries, scaled by the
    exchange chain measured at init) may fall either side: without SAENA_SINGLE_STREAM_NNZ it takes one stream or the kernel flags"""
    if G.variant()[0] == 5:
        return {"one-stream"}
    if EXPECT == "one-stream" and near_threshold:
        return {"one-stream", "kernel-flags"}
    return {EXPECT}


def through_wire(h, fp32):
    return h.astype(np.float32).astype(np.float64) if fp32 else h


# ---- one apply, four times back to back ---------------------------------------------------------------------------------------
def kinds(p):
    return ["spmv", "prolong_correct"] + (["residual", "residual_negative", "residual_multiply", "jacobi1", "chebyshev1"] if p.square else [])


def device_set(p, kind, v):
    d = {"x": capi.DeviceVector(p.N, v["x"])}
    if kind in ("jacobi1", "chebyshev1"):
        d["rhs"] = capi.DeviceVector(p.M, v["rhs"])
    elif kind == "prolong_correct":
        d["u"] = capi.DeviceVector(p.M, v["u"])
    else:
        d["y"] = capi.DeviceVector(p.M).fill(NAN)
        if kind != "spmv":
            d["rhs"] = capi.DeviceVector(p.M, v["rhs"])
        if kind == "residual_multiply":
            d["w"] = capi.DeviceVector(p.M, v["w"])
    return d


def launch(G, kind, d, v):
    """-> (the output, an input to overwrite behind the apply)"""
    if kind == "spmv":
        G.spmv(d["x"], d["y"])
    elif kind == "prolong_correct":
        G.prolong_correct(d["x"], d["u"])
        return d["u"], d["x"]
    elif kind == "residual":
        G.residual(d["x"], d["rhs"], d["y"])
    elif kind == "residual_negative":
        G.residual_negative(d["x"], d["rhs"], d["y"])
    elif kind == "residual_multiply":
        G.residual_multiply(d["x"], d["rhs"], d["y"], d["w"], v["c"])
    elif kind == "jacobi1":
        G.jacobi(1, d["x"], d["rhs"])
        return d["x"], d["rhs"]
    else:
        G.chebyshev(1, F.EIG, d["x"], d["rhs"])
        return d["x"], d["rhs"]
    return d["y"], d["x"]


def exchanged_outputs(X, p, kind, vs):
    sets = [device_set(p, kind, v) for v in vs]
    capi.check(capi.lib().sgpu_device_sync())
    outs = []
    for d, v in zip(sets, vs):                                  # nothing below waits for the device until the downloads
        o, spoil = launch(X, kind, d, v)
        spoil.fill(NAN)
        outs.append(o)
    return [o.download() for o in outs]


def twin_outputs(T, p, kind, vs, vi, fp32):
    outs = []
    for v in vs:
        T.debug_inject_halo(through_wire(v["x"][vi], fp32))
        d = device_set(p, kind, v)
        outs.append(launch(T, kind, d, v)[0].download())
    return outs


def epilogue(kind, s, v, invd):
    """the oracle's epilogues (oracle/saena_oracle.c) on a product s"""
    if kind == "spmv":
        return s
    if kind == "prolong_correct":
        return v["u"] - s
    if kind == "residual":
        return s - v["rhs"]
    if kind == "residual_negative":
        return v["rhs"] - s
    if kind == "residual_multiply":
        return (v["c"] * v["w"]) * (v["rhs"] - s)
    if kind == "jacobi1":
        return v["x"] - (s - v["rhs"]) * (invd * F.OMEGA)
    alpha, beta = 0.13 * F.EIG, F.EIG
    return v["x"] + (1.0 / ((beta + alpha) / 2.0)) * invd * (v["rhs"] - s)


def hold_to_contract(got, kind, s, b, v, invd, where):
    r = epilogue(kind, s, v, invd)
    if kind == "chebyshev1":
        assert np.linalg.norm(got - r) <= F.TOL_SWEEPS * np.linalg.norm(r), where
        return
    f = np.abs(v["c"] * v["w"]) if kind == "residual_multiply" else np.abs(F.OMEGA * invd) if kind == "jacobi1" else None
    lim = F.TOL * b * (1.0 if f is None else f) + 2 * F.EPS * np.abs(r) + 1e-300
    bad = np.flatnonzero(~(np.abs(got - r) <= lim))
    assert bad.size == 0, f"{where}: rows {bad[:10].tolist()} outside the bound"


# ---- a case under every form ---------------------------------------------------------------------------------------------------
def form_groups(all_forms):
    """forms grouped by the environment their builders read, each form in its own (tests/test_gpu_forms.py): one operator pair per
    group.  None: the form the operator comes up with, in the plain environment"""
    groups = {(): [None]}
    for f in (F.FORMS if all_forms else []):
        groups.setdefault(tuple(sorted(f.env.items())), []).append(f)
    return groups


def set_form(G, form):
    """-> None where the form serves the operator, else why not"""
    try:
        G.set_variant(form.variant)
    except capi.SgpuError as e:
        assert F.refused_as_documented(form, str(e)), (form.key, str(e))
        return "refused"
    if not F.name_matches(form, G.variant()[1]):
        return "another sub-form"
    G.set_lanes_per_row(form.lanes)
    if form.xw:
        try:
            G.set_x_windows(form.xw)
        except capi.SgpuError as e:
            assert F.X_WINDOWS_REFUSAL in str(e), str(e)
            return "refused"
    assert G.x_windows() == form.xw
    return None


def run_case(case, all_forms, served):
    p = mw.problem(case.problem)
    O = mw.mirror_oracle(p, case.mask)
    vi = mw.v_index(O)
    vs = [mw.case_vectors(p, k) for k in range(4)]
    invd = F.inv_diag(p) if p.square else None
    bound = [mw.abs_bound(p, v["x"]) for v in vs]
    out, modes = {}, set()
    if p.square:
        O.set_eig(F.EIG)
    for fp32 in (False, True):
        plain = [mw.apply_plain(p, v["x"], case.mask, fp32) for v in vs]
        O.set_use_double(not fp32)
        dense_f = None
        chain_ref = {}
        if p.square:
            x2, r2 = mw.twice(vs[0]["x"]), mw.twice(vs[0]["rhs"])
            chain_ref = {"jacobi4": mw.rank0(O, O.jacobi(4, x2, r2)), "chebyshev3": mw.rank0(O, O.chebyshev(3, x2, r2))}
        desc = mw.rank0_descriptor(O, fp32)
        for env, forms in form_groups(all_forms).items():
            for k, val in env:
                os.environ[k] = val
            try:
                X, T = capi.Operator(**desc), capi.Operator(**desc)
                for form in forms:
                    key = form.key if form else "default"
                    if form and (set_form(X, form) or set_form(T, form)):
                        continue
                    assert X.variant() == T.variant()
                    mode = X.exchange_mode()
                    assert mode in expected_modes(X, case.problem == "hub"), (case.name, key, mode, EXPECT)
                    modes.add(mode)
                    served.setdefault(key, set()).add(case.name)
                    where = f"{case.name}, {key}, fp32={fp32}"
                    s_ref = plain
                    if X.variant()[0] == 5 and fp32:            # the dense rows on the float wire round the whole of x (matvec_dense_float)
                        if dense_f is None:
                            dense_f = [mw.rank0(O, O.matvec_dense(mw.twice(v["x"]), as_float=True)) for v in vs]
                        s_ref = dense_f
                    for kind in kinds(p):
                        got = exchanged_outputs(X, p, kind, vs)
                        twin = twin_outputs(T, p, kind, vs, vi, fp32)
                        assert T.exchange_mode() == "none"
                        for k in range(4):
                            np.testing.assert_array_equal(F.bits(got[k]), F.bits(twin[k]), err_msg=f"{where}: {kind}, apply {k} of 4 against the twin")
                            hold_to_contract(twin[k], kind, s_ref[k], bound[k], vs[k], invd, f"{where}: the twin's {kind}, input {k}")
                        out[f"{key}/{'f32' if fp32 else 'f64'}/{kind}"] = digest(*got)
                    for name, ref in chain_ref.items():
                        du, dr = capi.DeviceVector(p.M, vs[0]["x"]), capi.DeviceVector(p.M, vs[0]["rhs"])
                        if name == "jacobi4":
                            X.jacobi(4, du, dr)
                        else:
                            X.chebyshev(3, F.EIG, du, dr)
                        dr.fill(NAN)
                        g = du.download()
                        if fp32:
                            assert np.max(np.abs(g - ref)) <= TOL_F32_CHAIN * np.max(np.abs(ref)), f"{where}: {name}"
                        else:
                            assert np.linalg.norm(g - ref) <= F.TOL_SWEEPS * np.linalg.norm(ref), f"{where}: {name}"
                        out[f"{key}/{'f32' if fp32 else 'f64'}/{name}"] = digest(g)
                if case.block and env == ():
                    run_block(case, p, O, X, T, vi, fp32, out)
                X.destroy(); T.destroy()
            finally:
                for k, _ in env:
                    os.environ.pop(k, None)
    return out, sorted(modes)


# ---- the block twin ------------------------------------------------------------------------------------------------------------
def fill_block(B, a):
    capi.check(capi.lib().sgpu_vec_fill(B.ptr, a, B.n * B.K))


def run_block(case, p, O, X, T, vi, fp32, out):
    """spmv_block and one Jacobi sweep, four inputs back to back with NaN written behind each apply, against inject_halo_block's bits;
    the twin's first input against the plain row loop, column by column; a 3-step Chebyshev against the 2-rank oracle"""
    n = p.M
    invd = F.inv_diag(p)
    for K in mw.BLOCK_K:
        Xs = [np.stack([inputs.v2(n, ofs=101 * j + 13 * k) * (1.0 + 0.25 * j) for j in range(K)], axis=1) for k in range(4)]
        Bs = [np.stack([inputs.rhs2(n, ofs=17 * j + 7 * k) + 0.5 * j for j in range(K)], axis=1) for k in range(4)]
        Xh, Bh = Xs[0], Bs[0]
        tag = f"block{K}/{'f32' if fp32 else 'f64'}"
        dB = capi.BlockVector(n, K, Bh)
        twin = []
        for Xk, Bk in zip(Xs, Bs):
            T.debug_inject_halo_block(through_wire(Xk[vi, :], fp32))
            dX, dY, dU, dR = capi.BlockVector(n, K, Xk), capi.BlockVector(n, K, np.full((n, K), NAN)), capi.BlockVector(n, K, Xk), capi.BlockVector(n, K, Bk)
            T.spmv_block(dX, dY)
            T.jacobi_block(1, dU, dR)
            twin.append((dY.download(), dU.download()))
        sets = [(capi.BlockVector(n, K, Xk), capi.BlockVector(n, K, np.full((n, K), NAN)), capi.BlockVector(n, K, Xk), capi.BlockVector(n, K, Bk))
                for Xk, Bk in zip(Xs, Bs)]
        capi.check(capi.lib().sgpu_device_sync())
        for dX, dY, dU, dR in sets:                             # nothing below waits for the device until the downloads
            X.spmv_block(dX, dY)
            fill_block(dX, NAN)
            X.jacobi_block(1, dU, dR)
            fill_block(dR, NAN)
        got = [(dY.download(), dU.download()) for _, dY, dU, _ in sets]
        for j in range(K):                                      # the twin itself: the forms' per-row bound, column by column
            s, b = mw.apply_plain(p, Xh[:, j], case.mask, fp32), mw.abs_bound(p, Xh[:, j])
            v = dict(x=Xh[:, j], rhs=Bh[:, j])
            hold_to_contract(twin[0][0][:, j], "spmv", s, b, v, invd, f"{case.name}, K={K}, fp32={fp32}: the twin's spmv_block, column {j}")
            hold_to_contract(twin[0][1][:, j], "jacobi1", s, b, v, invd, f"{case.name}, K={K}, fp32={fp32}: the twin's jacobi_block, column {j}")
        for k in range(4):
            for i, name in enumerate(("spmv_block", "jacobi_block")):
                np.testing.assert_array_equal(F.bits(got[k][i]), F.bits(twin[k][i]), err_msg=f"{case.name}, K={K}, fp32={fp32}: {name}, apply {k} of 4 against the twin")
        out[f"{tag}/spmv_block"] = digest(*[g[0] for g in got])
        out[f"{tag}/jacobi_block"] = digest(*[g[1] for g in got])
        dU = capi.BlockVector(n, K, Xh)
        X.chebyshev_block(3, F.EIG, dU, dB)
        g = dU.download()
        for j in range(K):
            ref = mw.rank0(O, O.chebyshev(3, mw.twice(Xh[:, j]), mw.twice(Bh[:, j])))
            if fp32:
                assert np.max(np.abs(g[:, j] - ref)) <= TOL_F32_CHAIN * np.max(np.abs(ref)), f"{case.name}, K={K}: chebyshev_block, column {j}"
            else:
                assert np.linalg.norm(g[:, j] - ref) <= F.TOL_SWEEPS * np.linalg.norm(ref), f"{case.name}, K={K}: chebyshev_block, column {j}"
        out[f"{tag}/chebyshev_block"] = digest(g)


# ---- hierarchies ---------------------------------------------------------------------------------------------------------------
def run_hierarchy(coarsest, coarse_solver):
    As, Ps, Rs = mw.hier()
    eig = hierarchy.eig_estimates(As)
    one = hierarchy.oracle_hierarchy(As, Ps, Rs)
    two = mw.mirror_hierarchy(As, Ps, Rs, coarsest)
    for a, e in zip(one[0], eig):
        a.set_eig(e)
    descs = mw.rank0_hierarchy(*two)
    n = As[0].shape[0]
    out, modes = {}, set()
    for smoother in ("jacobi", "chebyshev"):
        for pre, post in ((3, 3), (1, 0)):
            O1 = orc.OracleAmg(*one, pre=pre, post=post, smoother=smoother, max_iter=60, tol=1e-8)
            ops = [[capi.Operator(**d) for d in ds] for ds in descs]
            G = capi.Amg(*ops, eig_max=eig, pre=pre, post=post, smoother=smoother, max_iter=60, tol=1e-8, coarse_solver=coarse_solver)
            for ds, gs in zip(descs, ops):
                for d, g in zip(ds, gs):
                    mode = g.exchange_mode()
                    assert mode in (expected_modes(g) if "vIndex" in d else {"none"}), (mode, g.variant())
                    modes.add(mode)
            tag = f"{smoother}/{pre}+{post}"
            rhs, u0 = inputs.rhs2(n), inputs.v2(n) * 0.01
            want = O1.vcycle(u0, rhs)
            dr = capi.DeviceVector(n, rhs)
            runs = []
            for _ in range(3):                                  # (the first call may capture a graph, later ones replay it)
                du = capi.DeviceVector(n, u0)
                G.vcycle(du, dr)
                runs.append(du.download())
            assert np.linalg.norm(runs[0] - want) <= TOL_VCYCLE * np.linalg.norm(want), (tag, "vcycle")
            for r in runs[1:]:
                np.testing.assert_array_equal(F.bits(r), F.bits(runs[0]), err_msg=f"{tag}: V-cycle run to run")
            out[f"{tag}/vcycle"] = digest(runs[0])
            # (pCG does not reach 1e-8 within the 60 iterations under the one-sided (1, 0) cycle, in the oracle either: its 60 iterations
            # and its whole history are held like a converged one's)
            rhs = orc.laplacian3d_rhs(18)
            dr.upload(rhs)
            for name in ("solve", "solve_pCG"):
                _, it_o, h_o = getattr(O1, name)(rhs)
                runs = []
                for _ in range(2):
                    du = capi.DeviceVector(n)
                    it, h, conv = getattr(G, name)(du, dr)
                    runs.append((it, h, du.download()))
                it, h, u = runs[0]
                assert conv == bool(h_o[-1] <= 1e-8 * h_o[0]) and it == it_o and len(h) == len(h_o), (tag, name, conv, it, it_o)
                assert conv or (name, pre, post) == ("solve_pCG", 1, 0), (tag, name)
                assert np.all(np.abs(h - h_o) <= TOL_HIST * h_o[0]) and np.all(np.abs(h - h_o) <= 1e-6 * h_o), (tag, name, h, h_o)
                assert runs[1][0] == it, (tag, name)
                np.testing.assert_array_equal(F.bits(runs[1][1]), F.bits(h), err_msg=f"{tag}: {name} history run to run")
                np.testing.assert_array_equal(F.bits(runs[1][2]), F.bits(u), err_msg=f"{tag}: {name} iterate run to run")
                out[f"{tag}/{name}"] = digest(h, u)
            G.destroy()
    return out, sorted(modes)


def main():
    t_start = time.time()
    capi.init(0, 0, 1, capi.get_unique_id())
    capi.check(capi.lib().sgpu_barrier())
    served = {}
    for case in mw.catalogue():
        t0 = time.time()
        out, modes = run_case(case, case.forms, served)
        print(json.dumps(dict(case=case.name, modes=modes, seconds=round(time.time() - t0, 2), digests=out)), flush=True)
    print(json.dumps(dict(served={k: sorted(v) for k, v in served.items()})), flush=True)
    missing = [f.key for f in F.FORMS if f.key not in served]
    assert not missing, f"no operator of the catalogue ran {missing}"
    for name, coarsest, solver in (("hierarchy/coarsest-direct", False, "direct"), ("hierarchy/coarsest-CG", True, "CG")):
        t0 = time.time()
        out, modes = run_hierarchy(coarsest, solver)
        print(json.dumps(dict(case=name, modes=modes, seconds=round(time.time() - t0, 2), digests=out)), flush=True)
    capi.finalize()
    print(json.dumps(dict(seconds=round(time.time() - t_start, 2))), flush=True)
    print("RCCL_MIRROR_OK", flush=True)


if __name__ == "__main__":
    main()
