"""Time of the sensitivity evaluator on the bench batch, beside one solve of the same batch (developer tool,
needs the GPU).

The bench inputs (bench.make_inputs: config-2 x0 law, four shapes mixed per lane, the straight reference from
index 1) are solved by the fixed-K SQP-RTI from the controller's cold start (X = x0 repeated, U = 0), as
scripts/kkt_eval_rate.py does, so get('x'), get('u') and get('pi') pair with the references.  Then
  * qsp_eval_sens_device is timed with HIP events on device-resident copies of that iterate, after a warm-up
    and outside any copy: the median and minimum of --reps calls, K0 only and with dU (which adds the forward
    pass), with implied, given and no multipliers;
  * the feedback gains K0 of the first --lanes answers (implied multipliers) are summarised: largest entry per
    lane, and how many lanes have an input of stage 0 on a bound.

  python scripts/sens_rate.py [--batch 65536] [--N 20] [--sqp-iters 50] [--reps 7] [--lanes 4096] [--out FILE]
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
    d = dict(X=t(X), U=t(U), PI=t(PI), LAM=torch.zeros(B, N, 6, dtype=torch.float64, device=dev), yref=t(yref),
             shape_id=t(sid))
    o = dict(K0=torch.zeros(B, 2, 4, dtype=torch.float64, device=dev),
             dU=torch.zeros(B, N, 2, 4, dtype=torch.float64, device=dev),
             flag=torch.zeros(B, dtype=torch.int32, device=dev))
    # a stream of our own: the events and the launches must share it
    tstream = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    assert stream

    def timed(io):
        fn = lambda: s.eval_sens_device(io, stream=stream)
        fn()                                        # warm-up (allocates the handle's workspace)
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

    for name, mult, outs in (("given multipliers, K0 + flag", "given", ("K0", "flag")),
                             ("no multipliers, K0 + flag", "none", ("K0", "flag")),
                             ("implied multipliers, K0 + dU + flag", "implied", ("K0", "dU", "flag")),
                             ("implied multipliers, K0 + flag", "implied", ("K0", "flag"))):   # (last: checked below)
        io = _lib.SensIO()
        for k in ("X", "U", "shape_id"):
            setattr(io, k, d[k].data_ptr())
        if mult == "given":
            io.LAM = d["LAM"].data_ptr()
        if mult == "implied":
            io.PI, io.yref = d["PI"].data_ptr(), d["yref"].data_ptr()
        for k in outs:
            setattr(io, k, o[k].data_ptr())
        med, mn = timed(io)
        rec["rows"].append(dict(call=name, ms_median=med, ms_min=mn, lanes_per_s=B / (med * 1e-3),
                                share_of_the_solve=med / solve_ms, sqp_iterations_equivalent=med / (solve_ms / a.sqp_iters)))
        print(f"qsp_eval_sens_device, {name:38s} {med:8.4f} ms (min {mn:.4f})  {B / (med * 1e-3):.3e} lanes/s  "
              f"= {med / (solve_ms / a.sqp_iters):.3f} SQP iterations of this solve")
    torch.cuda.synchronize()

    # the gains of the fixed-K answers, implied multipliers, through the host entry
    r = s.eval_sens(X, U, PI=PI, want=("K0", "flag"))
    assert np.array_equal(r["K0"].view(np.uint64), o["K0"].cpu().numpy().view(np.uint64))   # host entry = device entry
    L = min(a.lanes, B)
    ok = (status[:L] == 0) & (r["flag"][:L] == 0)
    k0 = np.abs(r["K0"][:L][ok]).reshape(int(ok.sum()), -1).max(1)
    lh, uh = s._lh, s._uh
    on_bound = ((U[:L, 0] <= lh[1:] + 1e-6) | (U[:L, 0] >= uh[1:] - 1e-6))[ok]
    rec["gains"] = dict(lanes=L, used=int(ok.sum()), flagged=int(r["flag"][:L].sum()), max_abs_K0=dict(
        median=float(np.median(k0)), p90=float(np.percentile(k0, 90)), max=float(k0.max())),
        share_u_n0_on_a_bound=float(on_bound[:, 0].mean()), share_u_t0_on_a_bound=float(on_bound[:, 1].mean()),
        median_max_abs_K0_with_both_inputs_free=float(np.median(k0[~on_bound.any(1)])) if (~on_bound.any(1)).any() else None)
    print(f"K0 of the first {L} lanes (status 0 and finite: {int(ok.sum())}), implied multipliers: largest entry per lane "
          f"median {np.median(k0):.3e}, p90 {np.percentile(k0, 90):.3e}, max {k0.max():.3e}; stage-0 u_n on a bound on "
          f"{on_bound[:, 0].mean():.3f} of the lanes, u_t on {on_bound[:, 1].mean():.3f}; both free: median "
          f"{rec['gains']['median_max_abs_K0_with_both_inputs_free']}")
    s.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
