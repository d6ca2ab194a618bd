"""Time of the KKT evaluator on the bench batch, and the residuals of the fixed-K answers (developer tool,
needs the GPU).

The bench inputs (bench.make_inputs: config-2 x0 law, four shapes mixed per lane, the straight reference
from index 1) are solved by the fixed-K SQP-RTI from the controller's cold start (X = x0 repeated, U = 0),
which is the headline workload's solve without the warm-start shift, so get('x'), get('u') and get('pi') pair
with the references.  Then
  * qsp_eval_kkt_device is timed with HIP events on device-resident copies of that iterate, after a warm-up
    and outside any copy: the median and minimum of --reps calls, with implied and with given multipliers,
    with and without the optional parts / stage_res outputs;
  * the residuals of the first --lanes answers with implied multipliers are summarised per residual:
    median, 90th percentile, maximum, share below 1e-6.

  python scripts/kkt_eval_rate.py [--batch 65536] [--N 20] [--sqp-iters 50] [--reps 7] [--lanes 4096] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--sqp-iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from bench import SEED, SHAPES, make_inputs
    from uclv_qs_pushing_matlab_amd import _lib
    from uclv_qs_pushing_matlab_amd.objects import make_shape
    from uclv_qs_pushing_matlab_amd.solver import OcpSolver

    B, N = a.batch, a.N
    x0, yref, yref_e, sid, _ = make_inputs(B, N, SEED)
    s = OcpSolver(N=N, batch=B, sqp_iters=a.sqp_iters)
    s.set_shapes([make_shape(n) for n in SHAPES], shape_id=sid)
    s.set("constr_x0", x0)
    s.set("cost_y_ref", yref)
    s.set("cost_y_ref_e", yref_e)
    s.set("init_x", np.repeat(x0[:, None], N + 1, 1))
    s.set("init_u", np.zeros((B, N, 2)))
    s.solve()
    status = s.get("status")
    X, U, PI = s.get("x"), s.get("u"), s.get("pi")
    solve_ms = s.get("time_tot") * 1e3
    rec = dict(batch=B, N=N, sqp_iters=a.sqp_iters, reps=a.reps, solve_ms=solve_ms,
               ms_per_sqp_iteration_of_this_solve=solve_ms / a.sqp_iters, rows=[])
    print(f"solve: {solve_ms:.2f} ms for K = {a.sqp_iters} ({solve_ms / a.sqp_iters:.3f} ms per SQP iteration), "
          f"status 0 on {int((status == 0).sum())} of {B} lanes")

    dev = torch.device("cuda:0")
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    d = dict(x0=t(x0), X=t(X), U=t(U), PI=t(PI), LAM=torch.zeros(B, N, 6, dtype=torch.float64, device=dev),
             yref=t(yref), yref_e=t(yref_e), shape_id=t(sid))
    o = dict(res=torch.zeros(B, 4, dtype=torch.float64, device=dev),
             parts=torch.zeros(B, len(_lib.KKT_PARTS), dtype=torch.float64, device=dev),
             stage_res=torch.zeros(B, N + 1, 4, dtype=torch.float64, device=dev))
    # a stream of our own: the events and the launches must share it
    tstream = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    assert stream

    def timed(io):
        fn = lambda: s.eval_kkt_device(io, stream=stream)
        fn()                                        # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    for name, lam, outs in (("given multipliers, res only", True, ("res",)),
                            ("implied multipliers, res + parts + stage_res", False, ("res", "parts", "stage_res")),
                            ("implied multipliers, res only", False, ("res",))):   # (last: its res is checked below)
        io = _lib.KktIO()
        for k in ("x0", "X", "U", "PI", "yref", "yref_e", "shape_id"):
            setattr(io, k, d[k].data_ptr())
        io.LAM = d["LAM"].data_ptr() if lam else None
        for k in outs:
            setattr(io, k, o[k].data_ptr())
        med, mn = timed(io)
        rec["rows"].append(dict(call=name, ms_median=med, ms_min=mn, stages_per_s=B * (N + 1) / (med * 1e-3)))
        print(f"qsp_eval_kkt_device, {name:46s} {med:8.4f} ms (min {mn:.4f})  {B * (N + 1) / (med * 1e-3):.3e} stages/s")
    torch.cuda.synchronize()

    # residuals of the fixed-K answers, implied multipliers, through the host entry
    res, parts = s.eval_kkt(X, U, PI, "implied", x0=x0, yref=yref, yref_e=yref_e, parts=True)
    assert np.array_equal(res.view(np.uint64), o["res"].cpu().numpy().view(np.uint64))   # host entry = device entry
    L = min(a.lanes, B)
    ok = status[:L] == 0
    rec["residuals"] = dict(lanes=L, status0=int(ok.sum()), rows={})
    print(f"residuals of the first {L} lanes after K = {a.sqp_iters} (status 0 on {int(ok.sum())}), implied multipliers:")
    cols = [("res_stat", res[:L, 0]), ("res_eq", res[:L, 1]), ("res_ineq", res[:L, 2]), ("res_comp", res[:L, 3])]
    cols += [(k, parts[:L, i]) for i, k in enumerate(_lib.KKT_PARTS)]
    for k, v in cols:
        v = v[ok]
        row = dict(median=float(np.median(v)), p90=float(np.percentile(v, 90)), max=float(v.max()),
                   share_below_1e6=float((v < 1e-6).mean()))
        rec["residuals"]["rows"][k] = row
        print(f"  {k:10s} median {row['median']:.3e}  p90 {row['p90']:.3e}  max {row['max']:.3e}  below 1e-6: {row['share_below_1e6']:.3f}")
    s.close()

    # QP level: qsp_qp_solve's own status-0 answers on manufactured QPs with active state bounds (family Fs of
    # tests/manufactured_qp.py, N = 20), recomputed by qsp_qp_residuals -- the check that the header of
    # qsp_qp_solve sends its callers to
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import manufactured_qp as mq
    rec["qp"] = {}
    for fam in ("Fs", "Fs-small", "Fu"):
        q = mq.named_batch(fam, 20, 70)
        s = OcpSolver(N=20, batch=1, qp_iters=mq.QP_ITERS, mu_stop=mq.MU_STOP, stage0_s_bound=False)
        data = [q[k] for k in ("A", "B", "b", "H", "g", "lo", "hi", "dx0")]
        r = s.qp_solve(q["A"].reshape(70, 20, 16), q["B"].reshape(70, 20, 8), *data[2:])
        kk = s.qp_residuals(*data, r["dx"], r["du"], r["pi"], r["lam"])
        s.close()
        m = r["qp_status"] == 0
        row = {k: float(v[m].max()) for k, v in kk.items()}
        row["status0"] = int(m.sum())
        row["du_err"] = float(np.abs(r["du"][m] - q["du"][m]).max())
        rec["qp"][fam] = row
        print(f"qsp_qp_solve {fam:9s} N = 20: status 0 on {row['status0']} of 70; worst over them: " +
              "  ".join(f"{k} {row[k]:.2e}" for k in list(_lib.QP_RESIDUALS) + ["du_err"]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
